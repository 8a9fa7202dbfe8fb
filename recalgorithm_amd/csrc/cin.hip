// K5: xDeepFM CIN layer (algorithm/xDeepFM/cin_layer.py:4-30, xdeepfm.py:166-175) on the gfx950
// fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32, 64 FLOP/clk/SIMD).
//
//   X^{k+1}[b,n,d] = sum_{i,j} W[i*m+j, n] * X^k[b,i,d] * X^0[b,j,d]
//
// is an implicit GEMM  C[(b,d), n] = A[(b,d),(i,j)] * W[(i,j), n]  whose A operand
// A = X^k (x) X^0 (a Khatri-Rao product) is never materialised (the reference writes it to
// memory: 872 MB at B=4096, Hk=128 — cin_layer.py:21-22): every MFMA A-fragment element is
// produced in registers by one v_mul from a value of X^k and a value of X^0.
//
// One kernel, `cin_contract_kernel`, computes the generalised contraction
//   out[b,c,d] = sum_{p<HP} sum_{q<HQ} F[p*HQ+q, c] * P[b,p,d] * Q[b,q,d]
// and serves
//   forward : P = X^k, Q = X^0, F = W            -> X^{k+1}   (C = H_{k+1})
//   dX^k    : P = G,   Q = X^0, F = W' [n*m+j, i] -> dX^k      (C = H_k)
//   dX^0    : P = X^k, Q = G,   F = W''[i*N+n, j] -> dX^0      (C = m)
// (W', W'' are index permutations of W, made by cin_permute_kernel), and
// `cin_filter_grad_kernel` computes dW[(i,j),n] = sum_{(b,d)} A[(b,d),(i,j)] * G[(b,d),n]
// (split over the batch, deterministic second-pass sum).
//
// Fragment maps of v_mfma_f32_32x32x2_f32 (guides: cdna_hip_programming.md §3): lane l supplies
// A[row = l&31][k = l>>5] and B[k = l>>5][col = l&31]; acc reg r holds C[row = (r&3) + 8*(r>>2) +
// 4*(l>>5)][col = l&31].
#include <cstdlib>

#include "common.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kThreads = 256;     // 4 waves; one 32-row MFMA tile per wave
constexpr int kTM = 128;          // (b,d) rows per workgroup
constexpr int kQC = 32;           // q rows of F staged per slab

// ---------------------------------------------------------------------------------------------
// generalised contraction
// ---------------------------------------------------------------------------------------------
template <int D, int NT>
__global__ __launch_bounds__(kThreads, NT <= 2 ? 3 : 2) void cin_contract_kernel(
    const float* __restrict__ P, const float* __restrict__ Q, const float* __restrict__ F,
    unsigned B, unsigned HP, unsigned HQ, unsigned C, float* __restrict__ out, int accumulate,
    float* __restrict__ pool, unsigned pool_stride, unsigned pool_col) {
    constexpr unsigned EX = kTM / D;           // examples per workgroup
    constexpr unsigned CS = NT * 32;           // LDS row stride of an F slab (cols zero padded)
    const unsigned c0 = blockIdx.y * CS;       // first output column of this workgroup (column chunks of NT tiles)
    const unsigned Cl = min(CS, C - c0);       // columns of this chunk
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const unsigned HQp = (HQ + 1) & ~1u;
    const unsigned QS = HQp * D + 16;          // +16: the two examples of a 32-lane group hit disjoint banks
    float* Qs = smem;                          // [EX][QS]
    float* Fs = smem + EX * QS;                // [2][kQC][CS]

    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned hi = lane >> 5, l32 = lane & 31;
    const unsigned row = wave * 32 + l32;      // row of the workgroup tile this lane feeds as A
    const unsigned exl = row / D, dd = row % D;
    const unsigned b0 = blockIdx.x * EX;
    const unsigned b = b0 + exl;
    const bool valid = b < B;

    // ---- stage the Q tile (contiguous [EX][HQ][D] block of Q) and zero the F slabs ----------
    for (unsigned e = tid; e < EX * QS; e += kThreads) Qs[e] = 0.f;
    for (unsigned e = tid; e < 2 * kQC * CS; e += kThreads) Fs[e] = 0.f;
    __syncthreads();
    {
        const unsigned per_ex = HQ * D;
        for (unsigned e = tid; e < EX * per_ex; e += kThreads) {
            unsigned ex = e / per_ex, rem = e - ex * per_ex;
            if (b0 + ex < B) Qs[ex * QS + rem] = Q[(size_t)(b0 + ex) * per_ex + rem];
        }
    }
    const unsigned nqc = (HQ + kQC - 1) / kQC;             // slabs per p
    const unsigned nslab = HP * nqc;
    constexpr unsigned kStg = (kQC * CS + kThreads - 1) / kThreads;   // staged floats per thread
    float stg[kStg];
    auto slab_rows = [&](unsigned s) { unsigned qc = s % nqc; return min((unsigned)kQC, HQ - qc * kQC); };
    auto slab_src = [&](unsigned s) { unsigned p = s / nqc, qc = s % nqc; return F + ((size_t)p * HQ + (size_t)qc * kQC) * C; };
    auto stage_load = [&](unsigned s) {
        const float* src = slab_src(s) + c0;
        const unsigned n = slab_rows(s) * Cl;
#pragma unroll
        for (unsigned k = 0; k < kStg; ++k) {
            unsigned e = tid + k * kThreads;
            unsigned q = e / Cl, c = e - q * Cl;
            stg[k] = e < n ? src[(size_t)q * C + c] : 0.f;
        }
    };
    auto stage_store = [&](unsigned s, unsigned buf) {
        const unsigned n = slab_rows(s) * Cl;
        float* dst = Fs + buf * kQC * CS;
#pragma unroll
        for (unsigned k = 0; k < kStg; ++k) {
            unsigned e = tid + k * kThreads;
            if (e < n) {
                unsigned q = e / Cl, c = e - q * Cl;
                dst[q * CS + c] = stg[k];
            }
        }
    };
    stage_load(0);
    stage_store(0, 0);
    __syncthreads();

    // Two-level accumulation.  The reduction over (p, q) is HP * HQ terms long (3328 for the second layer of the
    // BASELINE configuration); one MFMA chain per output adds them strictly in order, i.e. with the rounding error of a
    // 3328-term sequential fp32 sum — 2-4 x more elements outside 1e-5 relative than the blocked GEMM of the reference's
    // CPU path leaves (profiles/r02z_strict_parity_all_gpu_tests.md).  The chain is cut every `flush_every` slabs
    // (~ 208 terms): the chunk sum goes to `tot` and a new chain starts from zero — error ~ sqrt(chunk) + sqrt(n / chunk)
    // instead of sqrt(n).  (`tot` doubles the accumulator registers: a workgroup covers NT <= 2 column tiles, wider
    // layers are column chunks over blockIdx.y.)
    f32x16 acc[NT], tot[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = tot[nt][r] = 0.f;
    const unsigned rows_per_slab = min(HQ, (unsigned)kQC);
    const unsigned flush_every = max(1u, (208u + rows_per_slab / 2) / rows_per_slab);
    unsigned since_flush = 0;

    const float* Pp = P + ((size_t)b * HP) * D + dd;       // P[b, p, dd] at stride D
    float a_p = valid ? Pp[0] : 0.f;
    const float* Qlane = Qs + exl * QS + dd;

    for (unsigned s = 0; s < nslab; ++s) {
        const unsigned buf = s & 1;
        const unsigned p = s / nqc, qc = s - p * nqc;
        const bool more = s + 1 < nslab;
        if (more) stage_load(s + 1);
        float a_next = a_p;
        if (more && qc + 1 == nqc && valid) a_next = Pp[(size_t)(p + 1) * D];   // next p's value
        const float* Fb = Fs + buf * kQC * CS + hi * CS + l32;
        const float* Qb = Qlane + (qc * kQC + hi) * D;
        const unsigned steps = (slab_rows(s) + 1) >> 1;
        for (unsigned qq = 0; qq < steps; ++qq) {
            float a = a_p * Qb[(2 * qq) * D];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                float bf = Fb[(2 * qq) * CS + nt * 32];
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bf, acc[nt], 0, 0, 0);
            }
        }
        if (more) {
            // the other buffer was last read in iteration s-1, i.e. before the previous barrier
            stage_store(s + 1, buf ^ 1);
        }
        if (++since_flush == flush_every || !more) {       // uniform over the workgroup
            since_flush = 0;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    tot[nt][r] += acc[nt][r];
                    acc[nt][r] = 0.f;
                }
        }
        a_p = a_next;
        __syncthreads();
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = tot[nt];

    // ---- epilogue: out[b, c, d] (float4 of 4 consecutive d) and the sum-pooling over d --------
    const unsigned R0 = blockIdx.x * kTM + wave * 32;      // first (b,d) row of this wave's tile
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const unsigned c = c0 + nt * 32 + l32;
        const bool cok = c < C;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const unsigned R = R0 + 8 * g4 + 4 * hi;
            const unsigned bb = R / D, d0 = R % D;
            if (cok && bb < B) {
                float4* o = reinterpret_cast<float4*>(out + ((size_t)bb * C + c) * D + d0);
                float4 v = make_float4(acc[nt][4 * g4 + 0], acc[nt][4 * g4 + 1], acc[nt][4 * g4 + 2], acc[nt][4 * g4 + 3]);
                if (accumulate) v = f4_add(v, *o);
                *o = v;
            }
        }
        if (pool) {
            if constexpr (D >= 8) {
                constexpr int EXW = 32 / D;                 // examples per wave tile
                constexpr int GPE = 4 / EXW;                // reg groups (of 4 rows x 2 halves) per example
#pragma unroll
                for (int e = 0; e < EXW; ++e) {
                    float sacc = 0.f;
#pragma unroll
                    for (int g = 0; g < GPE; ++g)
#pragma unroll
                        for (int r = 0; r < 4; ++r) sacc += acc[nt][4 * (e * GPE + g) + r];
                    sacc += __shfl_xor(sacc, 32, 64);
                    const unsigned bb = R0 / D + e;
                    if (hi == 0 && cok && bb < B) pool[(size_t)bb * pool_stride + pool_col + c] = sacc;
                }
            } else {                                        // D == 4: every (g4, hi) group is one example
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    float sacc = acc[nt][4 * g4] + acc[nt][4 * g4 + 1] + acc[nt][4 * g4 + 2] + acc[nt][4 * g4 + 3];
                    const unsigned bb = (R0 + 8 * g4 + 4 * hi) / D;
                    if (cok && bb < B) pool[(size_t)bb * pool_stride + pool_col + c] = sacc;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Round 5: the same contraction for the forward shapes of the benchmark (HQ = m <= 32 values of Q per row, C <= 128
// filter columns, float4-addressable filter), restructured after the lessons of tile_v2.h / profiles/r05_mfma_lab.md:
//   * a lane's Q values (X^0[b, q = 2 s + hi, d], NSTEP <= 16 of them) live in REGISTERS for the whole kernel: the A operand
//     of a step is one v_mul of two registers — no LDS read (the kernel above reads Q from LDS for every step);
//   * a workgroup covers ALL C <= 128 columns with NT sub-tiles interleaved along the columns (sub-tile j holds column
//     NT * l32 + j): ONE ds_read_b128 of the filter slab feeds the step's four MFMAs (above: one ds_read_b32 per MFMA, two
//     column chunks per layer each forming the outer-product operand again);
//   * a slab = the HQ filter rows of ONE p, staged as float4 (global -> registers three slabs ahead -> ds_write_b128) through a
//     3-slot LDS ring, ONE barrier per slab = per NSTEP * NT <= 52 MFMAs (above: per 32, with scalar loads and stores);
//   * every non-MFMA instruction is pinned behind a fixed MFMA (sched_barrier), the two-level accumulation is unchanged
//     (same flush period, same step order: the results are bit-identical to the kernel above).
// LDS instructions per MFMA: 0.25 + 8 tile stores per 52 (above: 1.5 + 16 scalar stores per 32).
// ---------------------------------------------------------------------------------------------
template <int D, int NT, int NSTEP>
__global__ __launch_bounds__(kThreads, 2) void cin_contract2_kernel(
    const float* __restrict__ P, const float* __restrict__ Q, const float* __restrict__ F, unsigned B, unsigned HP,
    unsigned HQ, unsigned C, float* __restrict__ out, int accumulate, float* __restrict__ pool, unsigned pool_stride,
    unsigned pool_col) {
    constexpr unsigned EX = kTM / D;           // examples per workgroup
    constexpr unsigned CS = NT * 32;           // LDS row stride of a slab (columns zero padded)
    constexpr unsigned QR = 2 * NSTEP;         // slab rows (q zero padded)
    constexpr unsigned kSlab = QR * CS;        // floats per ring slot
    constexpr unsigned kStg = (kSlab / 4 + kThreads - 1) / kThreads;     // staged float4 per thread and slab
    __shared__ __attribute__((aligned(16))) float Fs[3 * kSlab];
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned hi = lane >> 5, l32 = lane & 31;
    const unsigned row = wave * 32 + l32;      // row of the workgroup tile this lane feeds as A
    const unsigned exl = row / D, dd = row % D;
    const unsigned b = blockIdx.x * EX + exl;
    const bool valid = b < B;

    for (unsigned e = tid; e < 3 * kSlab / 4; e += kThreads) reinterpret_cast<float4*>(Fs)[e] = f4_zero();   // padding rows / columns stay 0
    float qreg[NSTEP];
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) {
        const unsigned q = 2 * s + hi;
        qreg[s] = (valid && q < HQ) ? Q[((size_t)b * HQ + q) * D + dd] : 0.f;
    }
    // slab p: rows [p * HQ, (p + 1) * HQ) of F, contiguous (row stride C), C % 4 == 0
    const unsigned n4 = HQ * C / 4;
    const unsigned C4 = C / 4;
    unsigned lds_off[kStg];
#pragma unroll
    for (unsigned k = 0; k < kStg; ++k) {
        const unsigned e = tid + k * kThreads;
        lds_off[k] = (e / C4) * CS + (e % C4) * 4;
    }
    auto stage_load = [&](unsigned p, float4 (&st)[kStg]) {
        const float4* src = reinterpret_cast<const float4*>(F + (size_t)min(p, HP - 1) * HQ * C);   // (slabs past the end: reloaded, never used)
#pragma unroll
        for (unsigned k = 0; k < kStg; ++k) {
            const unsigned e = tid + k * kThreads;
            st[k] = e < n4 ? src[e] : f4_zero();
        }
    };
    auto stage_store = [&](unsigned slot, const float4 (&st)[kStg], unsigned k) {
        if (tid + k * kThreads < n4) *reinterpret_cast<float4*>(Fs + slot * kSlab + lds_off[k]) = st[k];
    };
    float4 st0[kStg], st1[kStg];
    stage_load(0, st0);
    stage_load(1, st1);
    const float* Pp = P + ((size_t)b * HP) * D + dd;       // P[b, p, dd] at stride D
    float a_p = valid ? Pp[0] : 0.f;
    float a_n1 = (valid && HP > 1) ? Pp[D] : 0.f;          // p + 1
    __syncthreads();                                        // zero fill done
#pragma unroll
    for (unsigned k = 0; k < kStg; ++k) stage_store(0, st0, k);
#pragma unroll
    for (unsigned k = 0; k < kStg; ++k) stage_store(1, st1, k);
    stage_load(2, st0);
    __syncthreads();

    f32x16 acc[NT], tot[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = tot[nt][r] = 0.f;
    const unsigned rows_per_slab = min(HQ, (unsigned)kQC);
    const unsigned flush_every = max(1u, (208u + rows_per_slab / 2) / rows_per_slab);
    unsigned since_flush = 0;

    // operand values of one step: NT consecutive columns of slab row 2 s + hi
    struct FragB { float x[NT]; };
    auto read_frag = [&](unsigned slot, int s, FragB& f) {
        const float* ptr = Fs + slot * kSlab + (2 * s + hi) * CS + NT * l32;
        if constexpr (NT == 1) f.x[0] = ptr[0];
        else if constexpr (NT == 2) { const float2 v = *reinterpret_cast<const float2*>(ptr); f.x[0] = v.x; f.x[1] = v.y; }
        else { const float4 v = *reinterpret_cast<const float4*>(ptr); f.x[0] = v.x; f.x[1] = v.y; f.x[2] = v.z; f.x[3] = v.w; }
    };
    FragB fb[2], fnext;
    read_frag(0, 0, fb[0]);
    unsigned s0 = 0, s1 = 1, s2 = 2;                        // ring slots of slabs p, p+1, p+2
    auto step = [&](unsigned p, float4 (&cur)[kStg], float4 (&nxt)[kStg]) {
        float a_n2 = 0.f;
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) {
            const float a = a_p * qreg[s];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, fb[s & 1].x[j], acc[j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (j == 0) {
                    // fragments of the next step (the first step of the next slab goes to `fnext`: NSTEP may be odd)
                    if (s + 1 < NSTEP) read_frag(s0, s + 1, fb[(s + 1) & 1]);
                    else read_frag(s1, 0, fnext);
                }
                if (j == NT - 1) {
                    // global loads of slab p + 3 (steps 0 ..), P of p + 2 (step 1), registers of slab p + 2 -> LDS (from the middle on)
                    if (s < (int)kStg) {
                        const unsigned e = tid + s * kThreads;
                        const float4* src = reinterpret_cast<const float4*>(F + (size_t)min(p + 3, HP - 1) * HQ * C);
                        nxt[s] = e < n4 ? src[e] : f4_zero();
                    }
                    if (s == 1) a_n2 = (valid && p + 2 < HP) ? Pp[(size_t)(p + 2) * D] : 0.f;
                    constexpr int w0 = NSTEP / 2;
                    if (s >= w0 && s < w0 + (int)kStg) stage_store(s2, cur, s - w0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (++since_flush == flush_every || p + 1 == HP) {   // uniform over the workgroup
            since_flush = 0;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    tot[nt][r] += acc[nt][r];
                    acc[nt][r] = 0.f;
                }
        }
        fb[0] = fnext;
        a_p = a_n1;
        a_n1 = a_n2;
        const unsigned t = s0;
        s0 = s1; s1 = s2; s2 = t;
        __syncthreads();
    };
    static_assert((int)kStg <= NSTEP / 2 && NSTEP / 2 + (int)kStg <= NSTEP, "side-work slots");
    for (unsigned p = 0; p < HP; p += 2) {
        step(p, st0, st1);
        if (p + 1 < HP) step(p + 1, st1, st0);
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = tot[nt];

    // ---- epilogue: out[b, c, d] (float4 of 4 consecutive d) and the sum-pooling over d; column of (sub-tile nt, lane) = NT * l32 + nt
    const unsigned R0 = blockIdx.x * kTM + wave * 32;      // first (b,d) row of this wave's tile
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const unsigned c = NT * l32 + nt;
        const bool cok = c < C;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const unsigned R = R0 + 8 * g4 + 4 * hi;
            const unsigned bb = R / D, d0 = R % D;
            if (cok && bb < B) {
                float4* o = reinterpret_cast<float4*>(out + ((size_t)bb * C + c) * D + d0);
                float4 v = make_float4(acc[nt][4 * g4 + 0], acc[nt][4 * g4 + 1], acc[nt][4 * g4 + 2], acc[nt][4 * g4 + 3]);
                if (accumulate) v = f4_add(v, *o);
                *o = v;
            }
        }
        if (pool) {
            static_assert(D >= 8, "cin_contract2: D >= 8");
            constexpr int EXW = 32 / D;                 // examples per wave tile
            constexpr int GPE = 4 / EXW;                // reg groups (of 4 rows x 2 halves) per example
#pragma unroll
            for (int e = 0; e < EXW; ++e) {
                float sacc = 0.f;
#pragma unroll
                for (int g = 0; g < GPE; ++g)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sacc += acc[nt][4 * (e * GPE + g) + r];
                sacc += __shfl_xor(sacc, 32, 64);
                const unsigned bb = R0 / D + e;
                if (hi == 0 && cok && bb < B) pool[(size_t)bb * pool_stride + pool_col + c] = sacc;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// input gradients, fused: ONE implicit GEMM  dA^T[(i,j), (b,d)] = sum_n W[(i,j), n] * G[(b,d), n]
// (the gradient of the never-materialised outer product) whose tiles are consumed on the fly:
//   dX^k[b,i,d] = sum_j dA[(b,d),(i,j)] * X^0[b,j,d]     dX^0[b,j,d] = sum_i dA[(b,d),(i,j)] * X^k[b,i,d]
// i.e. half the matrix-core work of contracting dX^k and dX^0 separately.  Orientation: MFMA rows =
// j (one i per 32-row tile, j zero-padded to 32), MFMA columns = 32 (b,d) columns per wave, so that
//   * the B operand G[(b,d), n] of a wave never changes: it is loaded once into registers (N/2 VGPRs),
//   * sum_j is a lane-local sum over the 16 accumulator registers plus one cross-half shuffle,
//   * sum_i is a lane-local accumulation across tiles,
// and the only LDS traffic is one ds_read_b32 of the W tile per MFMA (row stride N+1: conflict free).
// Workgroup = 128 (b,d) columns (4 waves) sharing double-buffered W tiles; m <= 32, N <= 128.
// ---------------------------------------------------------------------------------------------
template <int D, int KS>
__global__ __launch_bounds__(kThreads) void cin_input_grad_kernel(
    const float* __restrict__ x0, const float* __restrict__ xk, const float* __restrict__ W,
    const float* __restrict__ G, unsigned B, unsigned m, unsigned Hk, unsigned N, float* __restrict__ dx0,
    int dx0_accumulate, float* __restrict__ dxk, int dxk_accumulate) {
    constexpr unsigned EX = kTM / D;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const unsigned NS = 2 * KS + 1;                  // LDS row stride of a W tile (k zero padded to 2*KS)
    float* Ws = smem;                                // [2][32][NS]
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned hi = lane >> 5, l32 = lane & 31;
    const unsigned col = wave * 32 + l32;
    const unsigned exl = col / D, dd = col % D;
    const unsigned b = blockIdx.x * EX + exl;
    const bool valid = b < B;

    for (unsigned e = tid; e < 2 * 32 * NS; e += kThreads) Ws[e] = 0.f;

    // B operand: G[b, n = 2s + hi, dd], register resident for the whole kernel
    float Breg[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const unsigned n = 2 * s + hi;
        Breg[s] = (valid && n < N) ? G[((size_t)b * N + n) * D + dd] : 0.f;
    }
    // X^0[b, j = acc_row(r, hi), dd] for this lane's column
    float x0v[16], dx0acc[16], dx0tot[16];            // (sum over i in chunks of 16: two-level, see cin_contract_kernel)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned j = (r & 3) + 8 * (r >> 2) + 4 * hi;
        x0v[r] = (valid && j < m) ? x0[((size_t)b * m + j) * D + dd] : 0.f;
        dx0acc[r] = dx0tot[r] = 0.f;
    }
    const unsigned tileN = m * N;                    // floats of one W tile (rows j < m, contiguous in W)
    constexpr unsigned kStg = (32 * 128 + kThreads - 1) / kThreads;
    float stg[kStg];
    auto stage_load = [&](unsigned i) {
        const float* src = W + (size_t)i * tileN;
#pragma unroll
        for (unsigned k = 0; k < kStg; ++k) {
            unsigned e = tid + k * kThreads;
            stg[k] = e < tileN ? src[e] : 0.f;
        }
    };
    auto stage_store = [&](unsigned buf) {
        float* dst = Ws + buf * 32 * NS;
#pragma unroll
        for (unsigned k = 0; k < kStg; ++k) {
            unsigned e = tid + k * kThreads;
            if (e < tileN) {
                unsigned j = e / N, n = e - j * N;
                dst[j * NS + n] = stg[k];
            }
        }
    };
    __syncthreads();                                 // zero fill done
    stage_load(0);
    stage_store(0);
    float xkv = valid ? xk[((size_t)b * Hk) * D + dd] : 0.f;
    __syncthreads();

    for (unsigned i = 0; i < Hk; ++i) {
        const unsigned buf = i & 1;
        const bool more = i + 1 < Hk;
        float xkv_next = 0.f;
        if (more) {
            stage_load(i + 1);
            if (valid) xkv_next = xk[((size_t)b * Hk + i + 1) * D + dd];
        }
        f32x16 accE, accO;
#pragma unroll
        for (int r = 0; r < 16; ++r) accE[r] = accO[r] = 0.f;
        const float* Wb = Ws + buf * 32 * NS + l32 * NS + hi;
#pragma unroll
        for (int s = 0; s < KS; s += 2) {
            accE = __builtin_amdgcn_mfma_f32_32x32x2f32(Wb[2 * s], Breg[s], accE, 0, 0, 0);
            accO = __builtin_amdgcn_mfma_f32_32x32x2f32(Wb[2 * s + 2], Breg[s + 1], accO, 0, 0, 0);
        }
        float dk = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float a = accE[r] + accO[r];       // dA[(b,d), (i, j = acc_row(r, hi))]
            dk = fmaf(a, x0v[r], dk);
            dx0acc[r] = fmaf(a, xkv, dx0acc[r]);
        }
        dk += __shfl_xor(dk, 32, 64);
        if (hi == 0 && valid) {
            float* p = dxk + ((size_t)b * Hk + i) * D + dd;
            *p = dxk_accumulate ? *p + dk : dk;
        }
        if (more) stage_store(buf ^ 1);              // last read before the previous barrier
        if ((i & 15) == 15 || !more) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                dx0tot[r] += dx0acc[r];
                dx0acc[r] = 0.f;
            }
        }
        xkv = xkv_next;
        __syncthreads();
    }
    if (valid) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned j = (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (j < m) {
                float* p = dx0 + ((size_t)b * m + j) * D + dd;
                *p = dx0_accumulate ? *p + dx0tot[r] : dx0tot[r];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Round 5: the fused input gradients for the benchmark's shapes (D = 16, m <= 32, N = 128, float4-addressable filter).
// Same implicit GEMM dA^T = W G^T consumed on the fly, other tile orientation and pipeline:
//   * MFMA rows = 32 consecutive i at ONE j (the kernel above: the m <= 32 values of j at one i, i.e. 26 of 32 rows used):
//     H_k = 128 is four full row blocks — 104 tiles per 128 columns instead of 128, 19 % fewer MFMAs;
//   * the W tile ([32 i][128 n], row stride m N in memory) is staged as float4 through a 3-slot LDS ring (row stride 132) and
//     fetched as ONE ds_read_b128 per four MFMA steps (above: scalar loads / stores, one ds_read_b32 per MFMA);
//   * the VALU consumption of tile t - 1 (dX^0[j] += sum_i dA X^k[i]; dX^k[i] += dA X^0[j]) runs in the shadow of tile t's
//     MFMAs on a second accumulator (above: behind the tile's own last MFMA, in front of a barrier);
//   * X^k of the lane's rows and the dX^k accumulators stay in registers: two passes of up to two row blocks each keep the
//     kernel under 256 registers (2 waves per SIMD); the second pass adds to dX^0 what the first one stored.
// ---------------------------------------------------------------------------------------------
constexpr int kLdW2 = 132;

template <int NIBP /* row blocks of 32 i per pass: 1 or 2 */>
__global__ __launch_bounds__(kThreads, 2) void cin_input_grad2_kernel(
    const float* __restrict__ x0, const float* __restrict__ xk, const float* __restrict__ W, const float* __restrict__ G,
    unsigned B, unsigned m, unsigned Hk, float* __restrict__ dx0, int dx0_accumulate, float* __restrict__ dxk,
    int dxk_accumulate) {
    constexpr unsigned D = 16, N = 128, EX = kTM / D;
    constexpr unsigned kTile = 32 * kLdW2;
    __shared__ __attribute__((aligned(16))) float Ws[3 * kTile];
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned hi = lane >> 5, l32 = lane & 31;
    const unsigned col = wave * 32 + l32;
    const unsigned exl = col / D, dd = col % D;
    const unsigned b = blockIdx.x * EX + exl;
    const bool valid = b < B;

    // B operand: G[b, n = 8 g + 4 hi + e, dd] for step 4 g + e, register resident for the whole kernel
    float Breg[64];
#pragma unroll
    for (int s = 0; s < 64; ++s) {
        const unsigned n = 8 * (s >> 2) + 4 * hi + (s & 3);
        Breg[s] = valid ? G[((size_t)b * N + n) * D + dd] : 0.f;
    }
    // staging: thread -> (row tid / 32 + 8 k, float4 column tid % 32) of a tile
    const unsigned sr = tid >> 5, sc = tid & 31;
    const unsigned nib_total = (Hk + 31) / 32;
    const unsigned npass = (nib_total + NIBP - 1) / NIBP;
    const float* Wl = Ws + l32 * kLdW2 + 4 * hi;              // + slot * kTile + 8 g
    const float* x0p = x0 + (size_t)b * m * D + dd;           // X^0[b, j, dd] at stride D

    for (unsigned pass = 0; pass < npass; ++pass) {
        const unsigned ib0 = pass * NIBP;                     // first row block of this pass
        const unsigned nib = min((unsigned)NIBP, nib_total - ib0);
        const unsigned ntiles = m * nib;                      // tile t: j = t / nib, row block ib0 + t % nib
        // X^k[b, i = 32 (ib0 + q) + acc_row(r, hi), dd] of this lane's column and the dX^k accumulators of the pass
        float xkv[NIBP][16], dxkacc[NIBP][16];
#pragma unroll
        for (int q = 0; q < NIBP; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned i = 32 * (ib0 + q) + (r & 3) + 8 * (r >> 2) + 4 * hi;
                xkv[q][r] = (valid && i < Hk) ? xk[((size_t)b * Hk + i) * D + dd] : 0.f;
                dxkacc[q][r] = 0.f;
            }
        float4 stg[4];
        auto tile_load = [&](unsigned t) {
            const unsigned tt = min(t, ntiles - 1);           // (tiles past the end: reloaded, never used)
            const unsigned j = tt / nib, ib = ib0 + tt % nib;
#pragma unroll
            for (unsigned k = 0; k < 4; ++k) {
                const unsigned i = 32 * ib + sr + 8 * k;
                stg[k] = i < Hk ? reinterpret_cast<const float4*>(W + ((size_t)i * m + j) * N)[sc] : f4_zero();
            }
        };
        auto tile_store = [&](unsigned slot, unsigned k) {
            *reinterpret_cast<float4*>(Ws + slot * kTile + (sr + 8 * k) * kLdW2 + sc * 4) = stg[k];
        };
        __syncthreads();                                      // (the previous pass is done with the ring)
        tile_load(0);
#pragma unroll
        for (unsigned k = 0; k < 4; ++k) tile_store(0, k);
        tile_load(1);
#pragma unroll
        for (unsigned k = 0; k < 4; ++k) tile_store(1, k);
        __syncthreads();
        f32x16 A, Pv;                                         // the tile being formed, the tile being consumed
#pragma unroll
        for (int r = 0; r < 16; ++r) Pv[r] = 0.f;
        float4 fa[2];
        fa[0] = *reinterpret_cast<const float4*>(Wl);
        unsigned s0 = 0, s1 = 1, s2 = 2;
        float dk = 0.f;
        float x0_prev = 0.f, x0_cur = valid ? x0p[0] : 0.f, x0_next = 0.f;    // X^0[b, j - 1 | j | j + 1, dd]
        // consume register r of the tile held in Pv: it belongs to row block qp and the j whose X^0 value is x0c.  Branch-free
        // in qp (wave-uniform, but a branch per slot would fence the schedule): the other row block gets an exact + 0
        auto consume = [&](int r, unsigned qp, float x0c) {
            if constexpr (NIBP == 1) {
                dk = fmaf(Pv[r], xkv[0][r], dk);
                dxkacc[0][r] = fmaf(Pv[r], x0c, dxkacc[0][r]);
            } else {
                const bool first = qp == 0;
                dk = fmaf(Pv[r], first ? xkv[0][r] : xkv[1][r], dk);
                dxkacc[0][r] = fmaf(Pv[r], first ? x0c : 0.f, dxkacc[0][r]);
                dxkacc[1][r] = fmaf(Pv[r], first ? 0.f : x0c, dxkacc[1][r]);
            }
        };
        auto finish_j = [&](unsigned j) {                     // every row block of j consumed: dX^0[b, j, dd] of this pass
            const float v = dk + __shfl_xor(dk, 32, 64);
            if (hi == 0 && valid) {
                float* pd = dx0 + ((size_t)b * m + j) * D + dd;
                *pd = (dx0_accumulate || pass > 0) ? *pd + v : v;
            }
            dk = 0.f;
        };
        unsigned q = 0, j = 0;                                // tile t = (j, row block q)
        for (unsigned t = 0; t < ntiles; ++t) {
            const unsigned qp = q == 0 ? nib - 1 : q - 1;     // row block of tile t - 1
            const float x0c = q == 0 ? x0_prev : x0_cur;      // and the X^0 value of its j
            const bool cons = t > 0;
            if (q == 0) x0_next = (valid && j + 1 < m) ? x0p[(size_t)(j + 1) * D] : 0.f;
            tile_load(t + 2);
            const float* rd = Wl + s0 * kTile;
            const float* rn = Wl + s1 * kTile;
#pragma unroll
            for (int g = 0; g < 16; ++g) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float av = e == 0 ? fa[g & 1].x : (e == 1 ? fa[g & 1].y : (e == 2 ? fa[g & 1].z : fa[g & 1].w));
                    if (g == 0 && e == 0) {
                        f32x16 z;
#pragma unroll
                        for (int r = 0; r < 16; ++r) z[r] = 0.f;
                        A = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Breg[0], z, 0, 0, 0);
                    } else {
                        A = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Breg[4 * g + e], A, 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    const int ls = 4 * g + e;                 // 0 .. 63
                    if (e == 0) {
                        if (g + 1 < 16) fa[(g + 1) & 1] = *reinterpret_cast<const float4*>(rd + 8 * (g + 1));
                        else fa[0] = *reinterpret_cast<const float4*>(rn);      // first group of the next tile
                    }
                    if (ls >= 8 && ls < 24 && cons) consume(ls - 8, qp, x0c);   // the previous tile: one register per slot
                    if (ls >= 40 && ls < 44) tile_store(s2, ls - 40);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (cons && q == 0) finish_j(j - 1);              // tile t - 1 was the last row block of j - 1
            Pv = A;                                           // (waits for the tile's last MFMA: ~1 % of a tile)
            if (++q == nib) { q = 0; ++j; x0_prev = x0_cur; x0_cur = x0_next; }
            const unsigned tmp = s0;
            s0 = s1; s1 = s2; s2 = tmp;
            __syncthreads();
        }
        // the last tile: (m - 1, nib - 1)
#pragma unroll
        for (int r = 0; r < 16; ++r) consume(r, nib - 1, x0_prev);
        finish_j(m - 1);
        // dX^k[b, i, dd] of the pass: lanes of both halves hold their own rows
        if (valid) {
#pragma unroll
            for (int q2 = 0; q2 < NIBP; ++q2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned i = 32 * (ib0 + q2) + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if ((unsigned)q2 < nib && i < Hk) {
                        float* pk = dxk + ((size_t)b * Hk + i) * D + dd;
                        *pk = dxk_accumulate ? *pk + dxkacc[q2][r] : dxkacc[q2][r];
                    }
                }
        }
    }
}

// F'[(a1*n2 + a2) * n0 + a0] = W[(a0*n1... see callers]  — generic 3-index permutation of the
// filter: dst[(x*NY + y)*NZ + z] = src[x*sx + y*sy + z*sz]
__global__ __launch_bounds__(256) void cin_permute_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                          unsigned NX, unsigned NY, unsigned NZ, unsigned sx,
                                                          unsigned sy, unsigned sz) {
    unsigned i = blockIdx.x * 256 + threadIdx.x;
    unsigned total = NX * NY * NZ;
    if (i >= total) return;
    unsigned z = i % NZ, t = i / NZ;
    unsigned y = t % NY, x = t / NY;
    dst[i] = src[(size_t)x * sx + (size_t)y * sy + (size_t)z * sz];
}

// G[b,n,d] = g_out[b,n,d] (or 0) + g_pool[b, n] (or 0)
template <int D>
__global__ __launch_bounds__(256) void cin_combine_grad_kernel(const float* __restrict__ g_out,
                                                               const float* __restrict__ g_pool,
                                                               unsigned pool_stride, unsigned pool_col,
                                                               unsigned total /* B*N */, unsigned N,
                                                               float* __restrict__ G) {
    constexpr int D4 = D / 4;
    unsigned i = blockIdx.x * 256 + threadIdx.x;     // over B*N*D4
    if (i >= total * D4) return;
    unsigned bn = i / D4;
    float4 v = g_out ? reinterpret_cast<const float4*>(g_out)[i] : f4_zero();
    if (g_pool) {
        unsigned bb = bn / N, n = bn - bb * N;
        float gp = g_pool[(size_t)bb * pool_stride + pool_col + n];
        v.x += gp; v.y += gp; v.z += gp; v.w += gp;
    }
    reinterpret_cast<float4*>(G)[i] = v;
}

// ---------------------------------------------------------------------------------------------
// filter gradient: dW[kk, c] = sum_r (P[r, kk / HQ] * Q[r, kk % HQ]) * G[r, c],  r = (b, d)
// workgroup = 128 rows kk (one 32-row MFMA tile per wave) x all C columns, over a slab of the
// batch (split-K over blockIdx.y); partial sums go to `partials[blockIdx.y][Kdim][C]`.
// ---------------------------------------------------------------------------------------------
// reduction rows (b,d) staged per chunk: RC = 128 when the Q tile is narrow (HQ <= 32: the BASELINE shapes), else 64
constexpr int kPW = 34;        // >= distinct p values touched by the 128 kk rows of a workgroup (m >= 4)

template <int D, int NT, int QI, int RC>
__global__ __launch_bounds__(kThreads, 2) void cin_filter_grad_kernel(
    const float* __restrict__ P, const float* __restrict__ Q, const float* __restrict__ G, unsigned B,
    unsigned HP, unsigned HQ, unsigned C, unsigned ex_per_split, float* __restrict__ partials) {
    constexpr unsigned EXC = RC / D;            // examples per chunk
    constexpr unsigned GS = NT * 32 + 4;         // LDS row strides
    constexpr unsigned GI = RC * NT * 32 / kThreads;          // staged G floats per thread
    constexpr unsigned PI = (RC * kPW + kThreads - 1) / kThreads;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Gs = smem;                            // [RC][GS]
    float* Ps = Gs + RC * GS;                   // [RC][kPW]
    float* Qs = Ps + RC * kPW;                  // [RC][HQ]
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned hi = lane >> 5, l32 = lane & 31;
    const unsigned Kdim = HP * HQ;
    const unsigned c0 = blockIdx.z * NT * 32;               // column chunk of this workgroup
    const unsigned Cl = min((unsigned)NT * 32, C - c0);
    const unsigned kk0 = blockIdx.x * 128;                  // first kk row of the workgroup
    const unsigned kk = kk0 + wave * 32 + l32;              // this lane's A' row
    const bool kok = kk < Kdim;
    const unsigned p_first = kk0 / HQ;
    const unsigned p_lane = kok ? kk / HQ : p_first, q_lane = kok ? kk % HQ : 0;
    const unsigned pp_lane = p_lane - p_first;              // column in Ps
    unsigned p_cnt = min(HP, (min(kk0 + 128, Kdim) - 1) / HQ + 1) - p_first;   // p values staged

    // two-level accumulation (see cin_contract_kernel): one chain per staged chunk of RC reduction rows, the chunk sums
    // added to `tot` — a split otherwise adds B * D / splits (3456 at the BASELINE shape) terms in one chain
    f32x16 acc[NT], tot[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = tot[nt][r] = 0.f;

    const unsigned ex_begin = blockIdx.y * ex_per_split;
    const unsigned ex_end = min(B, ex_begin + ex_per_split);
    // Chunks are prefetched global -> registers one chunk ahead, so that the HBM/L2 latency of chunk
    // c+1 is hidden under the MFMA loop of chunk c; only the register -> LDS transposing stores sit
    // between the two barriers.  The G and Q chunks are contiguous in memory ([b][c][d] over
    // consecutive b): float4 (4 consecutive d) per load.
    constexpr unsigned GI4 = GI / 4;
    float4 gst[GI4], qst[QI];
    float pst[PI];
    const unsigned per_ex4 = Cl * D / 4;                     // float4s of one example's column chunk (contiguous)
    const unsigned nG4 = EXC * per_ex4, nQ4 = EXC * HQ * D / 4, nP = EXC * p_cnt * D;
    auto prefetch = [&](unsigned e0) {
        const unsigned nex = min(EXC, ex_end - e0);
        const float4* gsrc = reinterpret_cast<const float4*>(G + ((size_t)e0 * C + c0) * D);
        const float4* qsrc = reinterpret_cast<const float4*>(Q + (size_t)e0 * HQ * D);
#pragma unroll
        for (unsigned k = 0; k < GI4; ++k) {
            const unsigned e = tid + k * kThreads;
            const unsigned ex = e / per_ex4, rem = e - ex * per_ex4;
            gst[k] = ex < nex ? gsrc[(size_t)ex * (C * D / 4) + rem] : f4_zero();
        }
#pragma unroll
        for (unsigned k = 0; k < QI; ++k) {
            const unsigned e = tid + k * kThreads;
            qst[k] = e < nex * HQ * D / 4 ? qsrc[e] : f4_zero();
        }
#pragma unroll
        for (unsigned k = 0; k < PI; ++k) {                 // P[b][p_first + pp][d]
            const unsigned e = tid + k * kThreads;
            const unsigned ex = e / (p_cnt * D), rem = e - ex * p_cnt * D;
            pst[k] = (e < nP && ex < nex) ? P[((size_t)(e0 + ex) * HP + p_first) * D + rem] : 0.f;
        }
    };
    auto commit = [&]() {                                   // registers -> LDS, transposed to [(ex,d)][col]
#pragma unroll
        for (unsigned k = 0; k < GI4; ++k) {
            const unsigned e4 = tid + k * kThreads;
            if (e4 < nG4) {
                const unsigned e = e4 * 4, d = e % D, t = e / D, c = t % Cl, ex = t / Cl;
                float* dst = Gs + (ex * D + d) * GS + c;
                dst[0] = gst[k].x; dst[GS] = gst[k].y; dst[2 * GS] = gst[k].z; dst[3 * GS] = gst[k].w;
            }
        }
#pragma unroll
        for (unsigned k = 0; k < QI; ++k) {
            const unsigned e4 = tid + k * kThreads;
            if (e4 < nQ4) {
                const unsigned e = e4 * 4, d = e % D, t = e / D, q = t % HQ, ex = t / HQ;
                float* dst = Qs + (ex * D + d) * HQ + q;
                dst[0] = qst[k].x; dst[HQ] = qst[k].y; dst[2 * HQ] = qst[k].z; dst[3 * HQ] = qst[k].w;
            }
        }
#pragma unroll
        for (unsigned k = 0; k < PI; ++k) {
            const unsigned e = tid + k * kThreads;
            if (e < nP) {
                const unsigned d = e % D, t = e / D, pp = t % p_cnt, ex = t / p_cnt;
                Ps[(ex * D + d) * kPW + pp] = pst[k];
            }
        }
    };
    if (ex_begin < ex_end) prefetch(ex_begin);
    unsigned chunks = 0;
    for (unsigned e0 = ex_begin; e0 < ex_end; e0 += EXC) {
        __syncthreads();                                    // previous chunk fully consumed
        commit();
        __syncthreads();
        if (e0 + EXC < ex_end) prefetch(e0 + EXC);
        const float* Pl = Ps + hi * kPW + pp_lane;
        const float* Ql = Qs + hi * HQ + q_lane;
        const float* Gl = Gs + hi * GS + l32;
#pragma unroll 4
        for (unsigned st = 0; st < RC / 2; ++st) {
            float a = kok ? Pl[(2 * st) * kPW] * Ql[(2 * st) * HQ] : 0.f;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                float bf = Gl[(2 * st) * GS + nt * 32];
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bf, acc[nt], 0, 0, 0);
            }
        }
        if ((++chunks & 3) == 0 || e0 + EXC >= ex_end) {     // chain length 4 chunks = 256 terms (uniform over the workgroup)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    tot[nt][r] += acc[nt][r];
                    acc[nt][r] = 0.f;
                }
        }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = tot[nt];
    // ---- write the partial tile: rows kk0 + wave*32 + (r&3) + 8*(r>>2) + 4*hi, col nt*32 + l32 ----
    float* pout = partials + (size_t)blockIdx.y * Kdim * C;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const unsigned c = c0 + nt * 32 + l32;
        if (c >= C) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            unsigned rr = kk0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (rr < Kdim) pout[(size_t)rr * C + c] = acc[nt][r];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Round 5: the filter gradient for the benchmark's shapes (D = 16, HQ = m <= 32, C <= 128 columns in 2 or 4 full tiles).
// The kernel above transposes every chunk of G, X^k and X^0 into [(b,d)][.] LDS tiles with scalar stores between two barriers
// (no MFMA in flight meanwhile) and issues 2 + NT ds_read_b32 per NT MFMAs.  Here the reduction index r = (b, d) is consumed
// in another order — step (b, u, e) contracts d = 4 u + e (lanes 0-31) and d = 8 + 4 u + e (lanes 32-63); any pairing of
// reduction indices is a valid fp32 chain as long as both operands use the same one — so that ONE ds_read_b128 of a tile
// kept in its GLOBAL layout [b][row][d] delivers a lane's operand values of four steps:
//   A: float4 of X^k[b, p(kk), 8 hi + 4 u ..] and of X^0[b, q(kk), ..], four v_mul;  B: float4 of G[b, c, 8 hi + 4 u ..] per tile
//   -> 2 + NT ds_read_b128 per 4 NT MFMAs (0.375 LDS instructions per MFMA at NT = 4; above: 2.0), tiles staged with
//   ds_write_b128 straight from the float4 global loads (row stride 20 floats: the 16 lanes served together hit 16
//   distinct 4-bank groups), a workgroup covers all C columns (the outer-product operand is formed once, not per column
//   chunk), 2-slot ring with ONE barrier per chunk of 2 examples = 16 NT MFMAs per wave, the next chunk's global loads and
//   LDS stores pinned into the MFMA shadow.  Two-level accumulation as above (chains of 256 terms).
// ---------------------------------------------------------------------------------------------
constexpr int kLdF2 = 20;      // LDS floats per [.][d] row (16 + 4)
constexpr int kPW2 = 10;       // >= distinct p values of a workgroup's 128 kk rows (HQ >= 17: 127 / 17 + 2 = 9)

template <int NT>
__global__ __launch_bounds__(kThreads, 2) void cin_filter_grad2_kernel(
    const float* __restrict__ P, const float* __restrict__ Q, const float* __restrict__ G, unsigned B, unsigned HP,
    unsigned HQ, unsigned C, unsigned ex_per_split, float* __restrict__ partials) {
    constexpr unsigned D = 16, EXC = 2, CS = NT * 32;
    constexpr unsigned kG = EXC * CS * kLdF2, kQ = EXC * 32 * kLdF2, kP = EXC * kPW2 * kLdF2;
    constexpr unsigned kSlot = kG + kQ + kP;
    constexpr unsigned GI = EXC * CS * 4 / kThreads;          // staged G float4 per thread (C == CS: exact)
    __shared__ __attribute__((aligned(16))) float smem[2 * kSlot];
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned hi = lane >> 5, l32 = lane & 31;
    const unsigned Kdim = HP * HQ;
    const unsigned kk0 = blockIdx.x * 128;
    const unsigned kk = min(kk0 + wave * 32 + l32, Kdim - 1);   // (rows past Kdim compute a copy of the last row; never stored)
    const unsigned p_first = kk0 / HQ;
    const unsigned p_lane = kk / HQ - p_first, q_lane = kk % HQ;
    const unsigned p_cnt = min(HP, (min(kk0 + 128, Kdim) - 1) / HQ + 1) - p_first;

    for (unsigned e = tid; e < 2 * kSlot / 4; e += kThreads) reinterpret_cast<float4*>(smem)[e] = f4_zero();   // rows c >= C stay 0

    f32x16 acc[NT], tot[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = tot[nt][r] = 0.f;

    const unsigned ex_begin = blockIdx.y * ex_per_split;
    const unsigned ex_end = min(B, ex_begin + ex_per_split);
    const unsigned C4 = C * 4;                                // float4 per example of G
    const unsigned nQ4 = EXC * HQ * 4, nP4 = EXC * p_cnt * 4;
    // this thread's staged pieces: GI float4 of G, one of Q (tid < nQ4), one of P (tid < nP4)
    unsigned g_ex[GI], g_rem[GI], g_dst[GI];
#pragma unroll
    for (unsigned k = 0; k < GI; ++k) {
        const unsigned e = tid + k * kThreads;
        g_ex[k] = e / C4; g_rem[k] = e % C4;
        g_dst[k] = (g_ex[k] * CS + g_rem[k] / 4) * kLdF2 + (g_rem[k] % 4) * 4;
    }
    const unsigned q_ex = tid / (HQ * 4), q_rem = tid % (HQ * 4);
    const unsigned q_dst = kG + (q_ex * 32 + q_rem / 4) * kLdF2 + (q_rem % 4) * 4;
    const unsigned p_ex = tid / (p_cnt * 4), p_rem = tid % (p_cnt * 4);
    const unsigned p_dst = kG + kQ + (p_ex * kPW2 + p_rem / 4) * kLdF2 + (p_rem % 4) * 4;
    float4 gst[GI], qst, pst;
    auto load_piece = [&](unsigned e0, unsigned k) {          // k < GI: G piece k; GI: Q; GI + 1: P
        if (k < GI) {
            const unsigned ex = e0 + g_ex[k];
            gst[k] = (g_ex[k] < EXC && ex < ex_end) ? reinterpret_cast<const float4*>(G + (size_t)ex * C * D)[g_rem[k]] : f4_zero();
        } else if (k == GI) {
            const unsigned ex = e0 + q_ex;
            qst = (tid < nQ4 && ex < ex_end) ? reinterpret_cast<const float4*>(Q + (size_t)ex * HQ * D)[q_rem] : f4_zero();
        } else {
            const unsigned ex = e0 + p_ex;
            pst = (tid < nP4 && ex < ex_end) ? reinterpret_cast<const float4*>(P + ((size_t)ex * HP + p_first) * D)[p_rem] : f4_zero();
        }
    };
    auto store_piece = [&](float* slot, unsigned k) {
        if (k < GI) { if (g_ex[k] < EXC) *reinterpret_cast<float4*>(slot + g_dst[k]) = gst[k]; }
        else if (k == GI) { if (tid < nQ4) *reinterpret_cast<float4*>(slot + q_dst) = qst; }
        else { if (tid < nP4) *reinterpret_cast<float4*>(slot + p_dst) = pst; }
    };
    constexpr unsigned kPieces = GI + 2;
    if (ex_begin < ex_end) {
#pragma unroll
        for (unsigned k = 0; k < kPieces; ++k) load_piece(ex_begin, k);
    }
    __syncthreads();                                          // zero fill done
#pragma unroll
    for (unsigned k = 0; k < kPieces; ++k) store_piece(smem, k);
    __syncthreads();

    // lane's read offsets inside a slot (floats): + example * stride + 4 u
    const unsigned offG = l32 * kLdF2 + 8 * hi;                               // + (ex * CS + 32 j) * kLdF2
    const unsigned offQ = kG + q_lane * kLdF2 + 8 * hi;                       // + ex * 32 * kLdF2
    const unsigned offP = kG + kQ + p_lane * kLdF2 + 8 * hi;                  // + ex * kPW2 * kLdF2
    struct Frag { float4 p, q, g[NT]; };
    auto read_frag = [&](const float* slot, unsigned grp, Frag& f) {          // grp = ex * 2 + u
        const unsigned ex = grp >> 1, u = grp & 1;
        f.p = *reinterpret_cast<const float4*>(slot + offP + ex * kPW2 * kLdF2 + 4 * u);
        f.q = *reinterpret_cast<const float4*>(slot + offQ + ex * 32 * kLdF2 + 4 * u);
#pragma unroll
        for (int j = 0; j < NT; ++j) f.g[j] = *reinterpret_cast<const float4*>(slot + offG + (ex * CS + 32 * j) * kLdF2 + 4 * u);
    };
    constexpr int NG = EXC * 2;                               // groups of 4 steps per chunk
    unsigned chunks = 0, cur = 0;
    Frag fr[2];
    read_frag(smem, 0, fr[0]);
    for (unsigned e0 = ex_begin; e0 < ex_end; e0 += EXC) {
        const float* rs = smem + cur * kSlot;
        float* ws = smem + (cur ^ 1) * kSlot;
        const bool more = e0 + EXC < ex_end;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const Frag& f = fr[g & 1];
            const float a[4] = {f.p.x * f.q.x, f.p.y * f.q.y, f.p.z * f.q.z, f.p.w * f.q.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const float bv = e == 0 ? f.g[j].x : (e == 1 ? f.g[j].y : (e == 2 ? f.g[j].z : f.g[j].w));
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], bv, acc[j], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    const int ls = e * NT + j;                // slot inside the group, 0 .. 4 NT - 1
                    // fragments of the next group of this chunk (the next chunk's first group is read behind the barrier)
                    if (ls == 0 && g + 1 < NG) read_frag(rs, g + 1, fr[(g + 1) & 1]);
                    // group 0: the next chunk's global loads; group NG - 1: registers -> the other slot
                    if (g == 0 && ls >= 1 && ls <= (int)kPieces && more) load_piece(e0 + EXC, ls - 1);
                    if (g == NG - 1 && ls < (int)kPieces && more) store_piece(ws, ls);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        static_assert((int)kPieces < 4 * NT, "side-work slots");
        if ((++chunks & 7) == 0 || !more) {                   // chains of 8 chunks = 256 terms (uniform over the workgroup)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    tot[nt][r] += acc[nt][r];
                    acc[nt][r] = 0.f;
                }
        }
        __syncthreads();
        cur ^= 1;
        if (more) read_frag(smem + cur * kSlot, 0, fr[0]);
    }
    // ---- write the partial tile: rows kk0 + wave*32 + (r&3) + 8*(r>>2) + 4*hi, col nt*32 + l32 ----
    float* pout = partials + (size_t)blockIdx.y * Kdim * C;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const unsigned c = nt * 32 + l32;
        if (c >= C) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            unsigned rr = kk0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (rr < Kdim) pout[(size_t)rr * C + c] = tot[nt][r];
        }
    }
}

__global__ __launch_bounds__(256) void cin_sum_partials_kernel(const float* __restrict__ partials, unsigned S,
                                                               size_t n, float* __restrict__ out) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float acc = 0.f;
    unsigned s = 0;
    for (; s + 4 <= S; s += 4) {                              // four independent loads in flight, added in split order
        const float a0 = partials[(size_t)s * n + i], a1 = partials[(size_t)(s + 1) * n + i];
        const float a2 = partials[(size_t)(s + 2) * n + i], a3 = partials[(size_t)(s + 3) * n + i];
        acc = (((acc + a0) + a1) + a2) + a3;
    }
    for (; s < S; ++s) acc += partials[(size_t)s * n + i];
    out[i] = acc;
}

// ---- host helpers ---------------------------------------------------------------------------
inline bool d_ok(int D) { return D == 4 || D == 8 || D == 16 || D == 32; }

inline size_t contract_smem(int D, int NT, int HQ) {
    unsigned HQp = (HQ + 1) & ~1u;
    return ((size_t)(kTM / D) * (HQp * D + 16) + 2 * (size_t)kQC * NT * 32) * sizeof(float);
}

template <int D, int NT>
int launch_contract_DN(const float* P, const float* Q, const float* F, int B, int HP, int HQ, int C, float* out,
                       int accumulate, float* pool, int pool_stride, int pool_col, hipStream_t st) {
    size_t smem = contract_smem(D, NT, HQ);
    dim3 grid(cdiv((int64_t)B * D, kTM), cdiv(C, NT * 32));
    RECALGO_CHECK(launch_lds<cin_contract_kernel<D, NT>>(grid, dim3(kThreads), smem, st, P, Q, F, (unsigned)B, (unsigned)HP,
            (unsigned)HQ, (unsigned)C, out, accumulate, pool, (unsigned)pool_stride, (unsigned)pool_col));
    return (int)hipGetLastError();
}

template <int D>
int launch_contract_D(int NT, const float* P, const float* Q, const float* F, int B, int HP, int HQ, int C,
                      float* out, int accumulate, float* pool, int pool_stride, int pool_col, hipStream_t st) {
    // column tiles per workgroup of the general kernel: at most 2 (128 registers with the two-level accumulators; wider layers
    // are column chunks over blockIdx.y — the benchmark's shapes take cin_contract2_kernel instead)
    if (NT == 1) return launch_contract_DN<D, 1>(P, Q, F, B, HP, HQ, C, out, accumulate, pool, pool_stride, pool_col, st);
    return launch_contract_DN<D, 2>(P, Q, F, B, HP, HQ, C, out, accumulate, pool, pool_stride, pool_col, st);
}

// out[b, c0:c0+C', d] for C' <= 128 per launch (column chunks of the filter are strided views, so
// chunking over C needs a compact filter: handled by the callers with C <= 128)
template <int D, int NT, int NSTEP>
int launch_contract2(const float* P, const float* Q, const float* F, int B, int HP, int HQ, int C, float* out, int accumulate,
                     float* pool, int pool_stride, int pool_col, hipStream_t st) {
    hipLaunchKernelGGL((cin_contract2_kernel<D, NT, NSTEP>), dim3(cdiv((int64_t)B * D, kTM)), dim3(kThreads), 0, st, P, Q, F,
                       (unsigned)B, (unsigned)HP, (unsigned)HQ, (unsigned)C, out, accumulate, pool, (unsigned)pool_stride,
                       (unsigned)pool_col);
    return (int)hipGetLastError();
}

int launch_contract(const float* P, const float* Q, const float* F, int B, int HP, int HQ, int C, int D, float* out,
                    int accumulate, float* pool, int pool_stride, int pool_col, hipStream_t st) {
    if (C <= 0 || C > 128) return (int)hipErrorInvalidValue;
    // the register-resident-Q kernel: emb width 16, 17 .. 32 fields (13 .. 16 steps per slab: at most 3 of 16 padded), filter
    // columns in whole float4s and in (32, 64] or (96, 128] (2 or 4 full column tiles); everything else takes the general kernel
    if (D == 16 && HQ > 16 && HQ <= 32 && C % 4 == 0 && aligned16(F) && HP >= 1 &&
        ((C > 32 && C <= 64) || (C > 96 && C <= 128))) {
        const bool wide = C > 64;
#define RECALGO_CIN2(NSTEP)                                                                                                          \
    return wide ? launch_contract2<16, 4, NSTEP>(P, Q, F, B, HP, HQ, C, out, accumulate, pool, pool_stride, pool_col, st)           \
                : launch_contract2<16, 2, NSTEP>(P, Q, F, B, HP, HQ, C, out, accumulate, pool, pool_stride, pool_col, st)
        if (HQ <= 26) { RECALGO_CIN2(13); }
        RECALGO_CIN2(16);
#undef RECALGO_CIN2
    }
    const int NT = cdiv(C, 32);
    switch (D) {
        case 4: return launch_contract_D<4>(NT, P, Q, F, B, HP, HQ, C, out, accumulate, pool, pool_stride, pool_col, st);
        case 8: return launch_contract_D<8>(NT, P, Q, F, B, HP, HQ, C, out, accumulate, pool, pool_stride, pool_col, st);
        case 16: return launch_contract_D<16>(NT, P, Q, F, B, HP, HQ, C, out, accumulate, pool, pool_stride, pool_col, st);
        case 32: return launch_contract_D<32>(NT, P, Q, F, B, HP, HQ, C, out, accumulate, pool, pool_stride, pool_col, st);
        default: return (int)hipErrorInvalidValue;
    }
}

template <int D, int KS>
int launch_input_grad_DK(const float* x0, const float* xk, const float* W, const float* G, int B, int m, int Hk, int N,
                         float* dx0, int dx0_acc, float* dxk, int dxk_acc, hipStream_t st) {
    const size_t smem = (size_t)2 * 32 * (2 * KS + 1) * sizeof(float);
    RECALGO_CHECK(launch_lds<cin_input_grad_kernel<D, KS>>(dim3(cdiv((int64_t)B * D, kTM)), dim3(kThreads), smem, st, x0, xk, W,
            G, (unsigned)B, (unsigned)m, (unsigned)Hk, (unsigned)N, dx0, dx0_acc, dxk, dxk_acc));
    return (int)hipGetLastError();
}
template <int D>
int launch_input_grad_D(const float* x0, const float* xk, const float* W, const float* G, int B, int m, int Hk, int N,
                        float* dx0, int dx0_acc, float* dxk, int dxk_acc, hipStream_t st) {
    const int ks = cdiv(cdiv(N, 2), 16) * 16;
    switch (ks) {
        case 16: return launch_input_grad_DK<D, 16>(x0, xk, W, G, B, m, Hk, N, dx0, dx0_acc, dxk, dxk_acc, st);
        case 32: return launch_input_grad_DK<D, 32>(x0, xk, W, G, B, m, Hk, N, dx0, dx0_acc, dxk, dxk_acc, st);
        case 48: return launch_input_grad_DK<D, 48>(x0, xk, W, G, B, m, Hk, N, dx0, dx0_acc, dxk, dxk_acc, st);
        case 64: return launch_input_grad_DK<D, 64>(x0, xk, W, G, B, m, Hk, N, dx0, dx0_acc, dxk, dxk_acc, st);
        default: return (int)hipErrorInvalidValue;
    }
}
int launch_input_grad(const float* x0, const float* xk, const float* W, const float* G, int B, int m, int Hk, int N,
                      int D, float* dx0, int dx0_acc, float* dxk, int dxk_acc, hipStream_t st) {
    switch (D) {
        case 4: return launch_input_grad_D<4>(x0, xk, W, G, B, m, Hk, N, dx0, dx0_acc, dxk, dxk_acc, st);
        case 8: return launch_input_grad_D<8>(x0, xk, W, G, B, m, Hk, N, dx0, dx0_acc, dxk, dxk_acc, st);
        case 16: return launch_input_grad_D<16>(x0, xk, W, G, B, m, Hk, N, dx0, dx0_acc, dxk, dxk_acc, st);
        case 32: return launch_input_grad_D<32>(x0, xk, W, G, B, m, Hk, N, dx0, dx0_acc, dxk, dxk_acc, st);
        default: return (int)hipErrorInvalidValue;
    }
}

inline int filter_rc(int /*HQ*/) { return 64; }          // (RC = 128 spills at NT = 2: 27 VGPRs, measured slower)
// the round-5 kernel (cin_filter_grad2_kernel): emb width 16, 17 .. 32 fields, all columns in one workgroup (C == 64 or 128)
inline bool filter_grad2_ok(int D, int HQ, int C) { return D == 16 && HQ > 16 && HQ <= 32 && (C == 64 || C == 128); }
inline int filter_grad_splits(int B, int D, int Kdim, int C, int HQ) {
    if (filter_grad2_ok(D, HQ, C)) {
        const int want = 512 / cdiv(Kdim, 128);             // one resident round of 2 workgroups per CU
        const int max_s = cdiv(B, 2);
        const int S = want < 1 ? 1 : (want > max_s ? max_s : want);
        return S > 128 ? 128 : S;                           // (the first layer: 6 row blocks x 85 splits of 50 examples)
    }
    int row_blocks = cdiv(Kdim, 128) * cdiv(C, 64);         // x column chunks of <= 2 tiles
    int want = 512 / row_blocks;                            // <= 2 workgroups per CU (VGPR-bound occupancy): no tail round
    int exc = filter_rc(HQ) / D;
    int max_s = cdiv(B, exc);
    int S = want < 1 ? 1 : (want > max_s ? max_s : want);
    return S > 64 ? 64 : S;
}

template <int D, int NT, int QI, int RC>
int launch_filter_grad_DNQ(const float* P, const float* Q, const float* G, int B, int HP, int HQ, int C, int S,
                           float* partials, hipStream_t st) {
    size_t smem = ((size_t)RC * (NT * 32 + 4) + (size_t)RC * kPW + (size_t)RC * HQ) * sizeof(float);
    const int exc = RC / D;
    int ex_per_split = cdiv(cdiv(B, S), exc) * exc;
    dim3 grid(cdiv(HP * HQ, 128), S, cdiv(C, NT * 32));
    RECALGO_CHECK(launch_lds<cin_filter_grad_kernel<D, NT, QI, RC>>(grid, dim3(kThreads), smem, st, P, Q, G, (unsigned)B,
            (unsigned)HP, (unsigned)HQ, (unsigned)C, (unsigned)ex_per_split, partials));
    return (int)hipGetLastError();
}
template <int D, int NT>
int launch_filter_grad_DN(const float* P, const float* Q, const float* G, int B, int HP, int HQ, int C, int S,
                          float* partials, hipStream_t st) {
    const int qi = cdiv(64 * HQ, 4 * kThreads);             // staged Q float4s per thread: HQ <= 32 | 64 | 128
    if (qi <= 2) return launch_filter_grad_DNQ<D, NT, 2, 64>(P, Q, G, B, HP, HQ, C, S, partials, st);
    if (qi <= 4) return launch_filter_grad_DNQ<D, NT, 4, 64>(P, Q, G, B, HP, HQ, C, S, partials, st);
    return launch_filter_grad_DNQ<D, NT, 8, 64>(P, Q, G, B, HP, HQ, C, S, partials, st);
}

template <int D>
int launch_filter_grad_D(int NT, const float* P, const float* Q, const float* G, int B, int HP, int HQ, int C, int S,
                         float* partials, hipStream_t st) {
    if (NT == 1) return launch_filter_grad_DN<D, 1>(P, Q, G, B, HP, HQ, C, S, partials, st);
    return launch_filter_grad_DN<D, 2>(P, Q, G, B, HP, HQ, C, S, partials, st);
}

struct BwdWs {
    size_t g, wp, wpp, partials, total;
};
inline BwdWs bwd_ws(int B, int m, int Hk, int N, int D) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    BwdWs w;
    size_t kdim = (size_t)Hk * m;
    w.g = 0;
    size_t off = al((size_t)B * N * D * sizeof(float));
    w.wp = off;   off += al(kdim * N * sizeof(float));
    w.wpp = off;  off += al(kdim * N * sizeof(float));
    w.partials = off;
    off += al((size_t)filter_grad_splits(B, D, (int)kdim, N, m) * kdim * N * sizeof(float));
    w.total = off;
    return w;
}

}  // namespace

// =============================================================================================
// C-ABI
// =============================================================================================
RECALGO_EXPORT int recalgo_cin_layer_fwd(const float* x0, const float* xk, const float* filters, int B, int m,
                                         int Hk, int N, int D, float* out, float* pool, int pool_stride,
                                         int pool_col, recalgo_stream_t stream) {
    RECALGO_REQUIRE(B >= 0 && m > 0 && Hk > 0 && N > 0 && N <= 128 && d_ok(D));
    if (B == 0) return 0;
    return launch_contract(xk, x0, filters, B, Hk, m, N, D, out, 0, pool, pool_stride, pool_col, as_stream(stream));
}

RECALGO_EXPORT int64_t recalgo_cin_layer_bwd_workspace_bytes(int B, int m, int Hk, int N, int D) {
    if (B <= 0 || m <= 0 || Hk <= 0 || N <= 0 || !d_ok(D)) return 0;
    return (int64_t)bwd_ws(B, m, Hk, N, D).total;
}

RECALGO_EXPORT int recalgo_cin_layer_bwd(const float* x0, const float* xk, const float* filters,
                                         const float* g_out, const float* g_pool, int pool_stride, int pool_col,
                                         int B, int m, int Hk, int N, int D, float* dx0, int dx0_accumulate,
                                         float* dxk, int dxk_accumulate, float* dfilters, void* workspace,
                                         recalgo_stream_t stream) {
    // m >= 4: the 128 kk rows of a filter-gradient workgroup touch at most 127 / m + 2 distinct p values, and Ps has kPW columns
    static_assert(127 / 4 + 2 <= kPW, "kPW holds the p values of a workgroup for every m >= 4");
    RECALGO_REQUIRE(B > 0 && m >= 4 && m <= 128 && Hk > 0 && Hk <= 128 && N > 0 && N <= 128 && d_ok(D));
    RECALGO_REQUIRE(workspace != nullptr && (g_out != nullptr || g_pool != nullptr));
    hipStream_t st = as_stream(stream);
    const BwdWs ws = bwd_ws(B, m, Hk, N, D);
    char* base = static_cast<char*>(workspace);
    float* G = reinterpret_cast<float*>(base + ws.g);
    float* Wp = reinterpret_cast<float*>(base + ws.wp);      // W' [n*m + j, i]
    float* Wpp = reinterpret_cast<float*>(base + ws.wpp);    // W''[i*N + n, j]
    float* partials = reinterpret_cast<float*>(base + ws.partials);
    const unsigned BN = (unsigned)B * N;
    // G = g_out + broadcast(g_pool)
    {
        const unsigned total4 = BN * (D / 4);
#define COMBINE(DD)                                                                                          \
    hipLaunchKernelGGL(cin_combine_grad_kernel<DD>, dim3(cdiv(total4, 256)), dim3(256), 0, st, g_out, g_pool, \
                       (unsigned)pool_stride, (unsigned)pool_col, BN, (unsigned)N, G)
        if (D == 4) COMBINE(4); else if (D == 8) COMBINE(8); else if (D == 16) COMBINE(16); else COMBINE(32);
#undef COMBINE
    }
    const unsigned wn = (unsigned)Hk * m * N;
    int rc;
    if (m <= 32 && dxk != nullptr && D == 16 && N == 128 && aligned16(filters)) {
        // fused, round-5 form: row blocks of 32 i (cin_input_grad2_kernel)
        const dim3 grid(cdiv((int64_t)B * D, kTM));
        if (Hk > 32) hipLaunchKernelGGL((cin_input_grad2_kernel<2>), grid, dim3(kThreads), 0, st, x0, xk, filters, G, (unsigned)B,
                                        (unsigned)m, (unsigned)Hk, dx0, dx0_accumulate, dxk, dxk_accumulate);
        else hipLaunchKernelGGL((cin_input_grad2_kernel<1>), grid, dim3(kThreads), 0, st, x0, xk, filters, G, (unsigned)B,
                                (unsigned)m, (unsigned)Hk, dx0, dx0_accumulate, dxk, dxk_accumulate);
        rc = (int)hipGetLastError();
        if (rc) return rc;
    } else if (m <= 32 && dxk != nullptr) {
        // fused: one implicit GEMM G W^T feeds both dX^k and dX^0 (cin_input_grad_kernel)
        rc = launch_input_grad(x0, xk, filters, G, B, m, Hk, N, D, dx0, dx0_accumulate, dxk, dxk_accumulate, st);
        if (rc) return rc;
    } else {
        // W[(i*m + j)*N + n] -> W'[(n*m + j)*Hk + i] : x=n, y=j, z=i
        hipLaunchKernelGGL(cin_permute_kernel, dim3(cdiv(wn, 256)), dim3(256), 0, st, filters, Wp, (unsigned)N,
                           (unsigned)m, (unsigned)Hk, 1u, (unsigned)N, (unsigned)(m * N));
        // W -> W''[(i*N + n)*m + j] : x=i, y=n, z=j
        hipLaunchKernelGGL(cin_permute_kernel, dim3(cdiv(wn, 256)), dim3(256), 0, st, filters, Wpp, (unsigned)Hk,
                           (unsigned)N, (unsigned)m, (unsigned)(m * N), 1u, (unsigned)N);
        // dX^k[b,i,d] = sum_{n,j} W'[(n,j), i] G[b,n,d] X0[b,j,d]
        if (dxk) {
            rc = launch_contract(G, x0, Wp, B, N, m, Hk, D, dxk, dxk_accumulate, nullptr, 0, 0, st);
            if (rc) return rc;
        }
        // dX^0[b,j,d] = sum_{i,n} W''[(i,n), j] X^k[b,i,d] G[b,n,d]
        rc = launch_contract(xk, G, Wpp, B, Hk, N, m, D, dx0, dx0_accumulate, nullptr, 0, 0, st);
        if (rc) return rc;
    }
    // dW
    const int S = filter_grad_splits(B, D, Hk * m, N, m);
    const int NT = cdiv(N, 32);
    if (filter_grad2_ok(D, m, N) && aligned16(G, x0, xk)) {
        const int ex_per_split = cdiv(cdiv(B, S), 2) * 2;
        const dim3 grid(cdiv(Hk * m, 128), S);
        if (N == 128) hipLaunchKernelGGL((cin_filter_grad2_kernel<4>), grid, dim3(kThreads), 0, st, xk, x0, G, (unsigned)B, (unsigned)Hk,
                                         (unsigned)m, (unsigned)N, (unsigned)ex_per_split, partials);
        else hipLaunchKernelGGL((cin_filter_grad2_kernel<2>), grid, dim3(kThreads), 0, st, xk, x0, G, (unsigned)B, (unsigned)Hk,
                                (unsigned)m, (unsigned)N, (unsigned)ex_per_split, partials);
        rc = (int)hipGetLastError();
    } else
    switch (D) {
        case 4: rc = launch_filter_grad_D<4>(NT, xk, x0, G, B, Hk, m, N, S, partials, st); break;
        case 8: rc = launch_filter_grad_D<8>(NT, xk, x0, G, B, Hk, m, N, S, partials, st); break;
        case 16: rc = launch_filter_grad_D<16>(NT, xk, x0, G, B, Hk, m, N, S, partials, st); break;
        default: rc = launch_filter_grad_D<32>(NT, xk, x0, G, B, Hk, m, N, S, partials, st); break;
    }
    if (rc) return rc;
    hipLaunchKernelGGL(cin_sum_partials_kernel, dim3(cdiv(wn, 256)), dim3(256), 0, st, partials, (unsigned)S, (size_t)wn,
                       dfilters);
    RECALGO_RETURN_LAST();
}
