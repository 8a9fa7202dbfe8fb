// PLE's "customized gate control" block (algorithm/PLE/extraction_network.py:25-85, algorithm/PLE/ple.py:185-226) at the
// reference's default sizes — 25 experts, gates of 15 and 25, 82 or 256 inputs — which csrc/mmoe.hip's gate_mix (E, n_g <= 16,
// 16 KiB of staged gate kernels, register arrays over E) does not serve.  include/recalgo_cgc.h states the contract:
//
//   z_g = x Wg,  p_g = softmax(z_g),  c[g][e] = sum_{j: sel[g][j] = e} p_g[j]
//   sum_outputs == 0:  out_g = sum_e c[g][e] expert_e          (G mix outputs)
//   sum_outputs != 0:  out   = sum_e (sum_g c[g][e]) expert_e  (ONE mix output: the tf.add_n of extraction_network.py:85)
//
// Both modes are ONE code path over M "mix outputs" (M = G, or 1) with coefficients cm[m][e]; the softmax side always sees
// the G real gates.  Backward: d_expert_e = sum_m cm[m][e] d_m, dp_g[j] = <d_m(g), expert_sel[g][j]> (M * E dot products at
// the most, only those a gate selects), dz_g = p_g (dp_g - <p_g, dp_g>), dx = sum_g dz_g Wg^T, dWg = x^T dz_g.
//
// Shape of both kernels: one wave64 per example row, EIGHT rows per 512-thread workgroup, the gate kernels staged once per
// workgroup in LDS (row stride NT | 1: lanes that walk k or c hit distinct banks), a persistent grid.  Nothing is indexed
// by E in registers: the experts are streamed four at a time (16-byte loads along H) into MMAX float4 accumulators
// (forward) or against MMAX held upstream chunks (backward).  Logits: a lane owns a gate column and walks k in double.
// dWg: each thread owns ceil(In * NT / 512) <= 40 (k, c) entries in REGISTERS over all rows of its workgroup (x and dz of
// the round's eight rows sit transposed in LDS: two 16-byte reads each per entry), written once as the workgroup's
// partial row; the step's deferred column sums add the rows in a fixed order.  No float atomics.
//
// Arms: MMAX in {1, 4, 8} >= M; VEC = every expert / output / gradient base pointer 16-byte aligned.
#include "common.h"

#include "../../include/recalgo_cgc.h"

namespace {

constexpr int kE = RECALGO_CGC_MAX_EXPERTS;            // E and n_g
constexpr int kG = RECALGO_CGC_MAX_GATES;
constexpr int kNT = kG * kE;                           // gate columns in all
constexpr int kMaxIn = 512;
constexpr int kWFloats = 20480;                        // LDS budget of the staged gate kernels: In * (NT | 1) floats (80 KiB)
constexpr int kRows = 8;                               // rows (= waves) per workgroup
constexpr int kThreads = 64 * kRows;
constexpr int kDw = kWFloats / kThreads;               // dWg entries a thread owns, at the most
constexpr int kFwdGrid = 512, kBwdGrid = 256;          // persistent grids: two / one workgroup per CU
constexpr int kTab = 2 * kG + 2 * kNT;                 // ints: n[G] | off[G] | gate of column c | expert of column c

struct CgcTables {
    const float* wg[kG];
    const float* ex[kE];
    int n[kG], off[kG];
    unsigned member[kG];            // per mix output: the experts some gate of it selects
    unsigned char sel[kNT];         // expert of gate column c
};
struct CgcFwdPtrs {
    float* out[kG];
};
struct CgcBwdPtrs {
    const float* dout[kG];
    float* dex[kE];
};

// gate kernels -> Ws[k * ldw + off_g + j]; tab = [n | off | gate of column | expert of column]
__device__ __forceinline__ void stage_gates(const CgcTables& T, int In, int G, int ldw, float* Ws, int* tab) {
    for (int g = 0; g < G; ++g) {
        const float* w = T.wg[g];
        const int n = T.n[g], off = T.off[g];
        for (int i = threadIdx.x; i < In * n; i += kThreads) {
            const int k = i / n, j = i - k * n;
            Ws[k * ldw + off + j] = w[i];
        }
        if ((int)threadIdx.x < n) {
            tab[2 * kG + off + threadIdx.x] = g;
            tab[2 * kG + kNT + off + threadIdx.x] = T.sel[off + threadIdx.x];
        }
        if (threadIdx.x == 0) tab[g] = n, tab[kG + g] = off;
    }
}

// cm[m * kE + e] = sum of the probabilities (ps: this row's) with which mix output m takes expert e, added in column order
__device__ __forceinline__ void mix_coefficients(const int* tab, const float* ps, float* cm, int E, int M, int NT, bool sum,
                                                 int lane) {
    for (int i = lane; i < M * kE; i += 64) {
        const int m = i / kE, e = i - m * kE;
        float a = 0.f;
        if (e < E) {
            const int c0 = sum ? 0 : tab[kG + m], c1 = sum ? NT : c0 + tab[m];
            for (int c = c0; c < c1; ++c) a += tab[2 * kG + kNT + c] == e ? ps[c] : 0.f;
        }
        cm[i] = a;
    }
}

template <int MMAX, bool VEC>
__global__ __launch_bounds__(kThreads) void cgc_fwd_kernel(CgcTables T, CgcFwdPtrs O, const float* __restrict__ x, int ldx,
                                                           int B, int In, int E, int G, int H, int NT, int sum,
                                                           float* __restrict__ p_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int ldw = NT | 1, NT4 = round4(NT), In4 = round4(In);
    const int M = sum ? 1 : G;
    float* Ws = reinterpret_cast<float*>(smem);
    int* tab = reinterpret_cast<int*>(Ws + round4(In * ldw));
    float* wave_s = reinterpret_cast<float*>(tab + kTab);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* zs = reinterpret_cast<double*>(wave_s + wave * (5 * NT4 + In4 + MMAX * kE));       // logits
    double* es = zs + NT4;                                                                     // exp(z - max)
    float* ps = reinterpret_cast<float*>(es + NT4);
    float* xs = ps + NT4;
    float* cm = xs + In4;
    stage_gates(T, In, G, ldw, Ws, tab);
    __syncthreads();
    const int H4 = H >> 2;
    for (int row = blockIdx.x * kRows + wave; row < B; row += gridDim.x * kRows) {
        for (int k = lane; k < In; k += 64) xs[k] = x[(size_t)row * ldx + k];
        wave_sync();
        // z = x Wg: a lane owns a gate column and walks k.  The logits and their softmax are NT numbers per row: evaluated in
        // double (a logit of magnitude 80 carries 4e-6 of rounding per fp32 operation, which the softmax turns into that much
        // RELATIVE error of every probability and of everything the backward derives from them; csrc/mmoe.hip)
        for (int c = lane; c < NT; c += 64) {
            double s = 0.0;
            for (int k = 0; k < In; ++k) s = fma((double)xs[k], (double)Ws[k * ldw + c], s);
            zs[c] = s;
        }
        wave_sync();
        for (int c = lane; c < NT; c += 64) {
            const int g = tab[2 * kG + c], n = tab[g], off = tab[kG + g];
            double m = zs[off];
            for (int j = 1; j < n; ++j) m = fmax(m, zs[off + j]);
            es[c] = exp(zs[c] - m);
        }
        wave_sync();
        for (int c = lane; c < NT; c += 64) {
            const int g = tab[2 * kG + c], n = tab[g], off = tab[kG + g];
            double s = 0.0;
            for (int j = 0; j < n; ++j) s += es[off + j];        // (every lane of the gate adds in the same order)
            const float p = (float)(es[c] / s);
            ps[c] = p;
            p_out[(size_t)row * NT + c] = p;
        }
        wave_sync();
        mix_coefficients(tab, ps, cm, E, M, NT, sum != 0, lane);
        wave_sync();
        for (int i = lane; i < H4; i += 64) {
            const size_t at = (size_t)row * H + 4 * i;
            float4 acc[MMAX];
#pragma unroll
            for (int m = 0; m < MMAX; ++m) acc[m] = f4_zero();
            for (int e0 = 0; e0 < E; e0 += 4) {
                float4 ev[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) ev[u] = e0 + u < E ? ld4<VEC>(T.ex[e0 + u] + at) : f4_zero();
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (e0 + u < E) {
#pragma unroll
                        for (int m = 0; m < MMAX; ++m)
                            if (m < M) acc[m] = f4_fma(ev[u], cm[m * kE + e0 + u], acc[m]);
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < MMAX; ++m)
                if (m < M) st4<VEC>(O.out[m] + at, acc[m]);
        }
        wave_sync();             // (the next row overwrites xs / ps / cm)
    }
}

template <int MMAX, bool VEC>
__global__ __launch_bounds__(kThreads) void cgc_bwd_kernel(CgcTables T, CgcBwdPtrs P, const float* __restrict__ x, int ldx,
                                                           const float* __restrict__ p_in, int B, int In, int E, int G, int H,
                                                           int NT, int sum, int relu_experts, float* __restrict__ dx, int lddx,
                                                           float* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int ldw = NT | 1, NT4 = round4(NT), In4 = round4(In);
    const int M = sum ? 1 : G;
    float* Ws = reinterpret_cast<float*>(smem);
    int* tab = reinterpret_cast<int*>(Ws + round4(In * ldw));
    float* xT = reinterpret_cast<float*>(tab + kTab);      // [In4][kRows]: x of the round's rows
    float* dzT = xT + In4 * kRows;                         // [NT4][kRows]: dz of the round's rows
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* ps = dzT + NT4 * kRows + wave * (NT4 + 2 * MMAX * kE);
    float* cm = ps + NT4;
    float* dpe = cm + MMAX * kE;                           // [m][e]: <d_m, expert_e>
    stage_gates(T, In, G, ldw, Ws, tab);
    float acc[kDw];                                        // this thread's dWg entries idx = threadIdx.x + i * kThreads
#pragma unroll
    for (int i = 0; i < kDw; ++i) acc[i] = 0.f;
    const int total = In * NT;
    const int k0 = threadIdx.x / NT, c0 = threadIdx.x - k0 * NT, kq = kThreads / NT, cr = kThreads - kq * NT;
    __syncthreads();
    const int H4 = H >> 2, passes = (H4 + 63) >> 6;
    const int rounds = (B + gridDim.x * kRows - 1) / (gridDim.x * kRows);
    for (int r = 0; r < rounds; ++r) {
        const int row = (r * gridDim.x + blockIdx.x) * kRows + wave;
        const bool valid = row < B;                      // (wave-uniform; a wave without a row adds exact zeros to dWg)
        for (int c = lane; c < NT; c += 64) {
            ps[c] = valid ? p_in[(size_t)row * NT + c] : 0.f;
            dzT[c * kRows + wave] = 0.f;
        }
        for (int k = lane; k < In; k += 64) xT[k * kRows + wave] = valid ? x[(size_t)row * ldx + k] : 0.f;
        for (int i = lane; i < M * kE; i += 64) dpe[i] = 0.f;
        wave_sync();
        if (valid) {
            mix_coefficients(tab, ps, cm, E, M, NT, sum != 0, lane);
            wave_sync();
            for (int pass = 0; pass < passes; ++pass) {
                const int i = pass * 64 + lane;
                const bool on = i < H4;                  // (every lane stays in the loop: it holds wave sums)
                const size_t at = (size_t)row * H + 4 * (on ? i : 0);
                float4 dg[MMAX];
#pragma unroll
                for (int m = 0; m < MMAX; ++m)
                    dg[m] = (m < M && on && P.dout[m] != nullptr) ? ld4<VEC>(P.dout[m] + at) : f4_zero();
                for (int e0 = 0; e0 < E; e0 += 4) {
                    float4 ev[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) ev[u] = (e0 + u < E && on) ? ld4<VEC>(T.ex[e0 + u] + at) : f4_zero();
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int e = e0 + u;
                        if (e < E) {
                            float4 de = f4_zero();
#pragma unroll
                            for (int m = 0; m < MMAX; ++m) {
                                if (m < M) {
                                    de = f4_fma(dg[m], cm[m * kE + e], de);
                                    if ((T.member[m] >> e) & 1u) {
                                        const float s = wave_sum(f4_dot(dg[m], ev[u]));
                                        if (lane == 0) dpe[m * kE + e] += s;
                                    }
                                }
                            }
                            float* out = P.dex[e];
                            if (out != nullptr && on) {
                                if (relu_experts) {
                                    de.x = ev[u].x > 0.f ? de.x : 0.f, de.y = ev[u].y > 0.f ? de.y : 0.f;
                                    de.z = ev[u].z > 0.f ? de.z : 0.f, de.w = ev[u].w > 0.f ? de.w : 0.f;
                                }
                                st4<VEC>(out + at, de);
                            }
                        }
                    }
                }
            }
            wave_sync();
            for (int c = lane; c < NT; c += 64) {        // dz of gate column c
                const int g = tab[2 * kG + c], n = tab[g], off = tab[kG + g];
                const float* dp = dpe + (sum ? 0 : g) * kE;
                const int* sel = tab + 2 * kG + kNT;
                float s = 0.f;
                for (int j = 0; j < n; ++j) s = fmaf(ps[off + j], dp[sel[off + j]], s);
                dzT[c * kRows + wave] = ps[c] * (dp[sel[c]] - s);
            }
            wave_sync();
            if (dx != nullptr) {
                for (int k = lane; k < In; k += 64) {
                    float s = 0.f;
                    for (int c = 0; c < NT; ++c) s = fmaf(dzT[c * kRows + wave], Ws[k * ldw + c], s);
                    dx[(size_t)row * lddx + k] = s;
                }
            }
        }
        __syncthreads();
        // dWg += x^T dz over the round's eight rows, in row order
        {
            int k = k0, c = c0;
#pragma unroll
            for (int i = 0; i < kDw; ++i) {
                if ((int)threadIdx.x + i * kThreads < total) {
                    const float4 xa = *reinterpret_cast<const float4*>(xT + k * kRows);
                    const float4 xb = *reinterpret_cast<const float4*>(xT + k * kRows + 4);
                    const float4 da = *reinterpret_cast<const float4*>(dzT + c * kRows);
                    const float4 db = *reinterpret_cast<const float4*>(dzT + c * kRows + 4);
                    float a = acc[i];
                    a = fmaf(xa.x, da.x, a), a = fmaf(xa.y, da.y, a), a = fmaf(xa.z, da.z, a), a = fmaf(xa.w, da.w, a);
                    a = fmaf(xb.x, db.x, a), a = fmaf(xb.y, db.y, a), a = fmaf(xb.z, db.z, a), a = fmaf(xb.w, db.w, a);
                    acc[i] = a;
                }
                c += cr, k += kq;
                if (c >= NT) c -= NT, ++k;
            }
        }
        __syncthreads();
    }
    // partials[block][In * off_g + k * n_g + j]: gate g's [In, n_g] kernel gradient is one contiguous run of the row
    float* prow = partials + (size_t)blockIdx.x * total;
    int k = k0, c = c0;
#pragma unroll
    for (int i = 0; i < kDw; ++i) {
        if ((int)threadIdx.x + i * kThreads < total) {
            const int g = tab[2 * kG + c], n = tab[g], off = tab[kG + g];
            prow[In * off + k * n + (c - off)] = acc[i];
        }
        c += cr, k += kq;
        if (c >= NT) c -= NT, ++k;
    }
}

struct CgcShape {
    int NT, M, mmax;
    bool vec;
};

size_t fwd_lds(int In, int NT, int mmax) {
    return sizeof(float) * (size_t)(round4(In * (NT | 1)) + kTab + kRows * (5 * round4(NT) + round4(In) + mmax * kE));
}
size_t bwd_lds(int In, int NT, int mmax) {
    return sizeof(float) * (size_t)(round4(In * (NT | 1)) + kTab + kRows * (round4(In) + round4(NT)) +
                                    kRows * (round4(NT) + 2 * mmax * kE));
}

bool limits_ok(int In, int E, int G, int H, int64_t NT, int n_max) {
    return In >= 1 && In <= kMaxIn && E >= 1 && E <= kE && G >= 1 && G <= kG && H >= 4 && (H & 3) == 0 && n_max >= 1 &&
           n_max <= kE && NT >= G && NT <= (int64_t)G * n_max && (int64_t)In * (NT | 1) <= kWFloats &&
           fwd_lds(In, (int)NT, kG) <= kLdsMax && bwd_lds(In, (int)NT, kG) <= kLdsMax;
}

// validates the tables and fills T; -> false outside the served limits
bool cgc_tables(const float* const* gate_kernels, const int* n_sel, const int* sel, const float* const* experts, int B, int In,
                int E, int G, int H, int sum, CgcTables* T, CgcShape* S) {
    if (!gate_kernels || !n_sel || !sel || !experts || B < 1 || G < 1 || G > kG) return false;
    int NT = 0, n_max = 0;
    for (int g = 0; g < G; ++g) {
        if (n_sel[g] < 1 || n_sel[g] > kE) return false;
        NT += n_sel[g];
        n_max = n_sel[g] > n_max ? n_sel[g] : n_max;
    }
    if (!limits_ok(In, E, G, H, NT, n_max)) return false;
    *T = CgcTables{};
    const int M = sum ? 1 : G;
    bool vec = true;
    int c = 0;
    for (int g = 0; g < G; ++g) {
        if (gate_kernels[g] == nullptr) return false;
        T->wg[g] = gate_kernels[g], T->n[g] = n_sel[g], T->off[g] = c;
        for (int j = 0; j < n_sel[g]; ++j, ++c) {
            if (sel[c] < 0 || sel[c] >= E) return false;
            T->sel[c] = (unsigned char)sel[c];
            T->member[sum ? 0 : g] |= 1u << sel[c];
        }
    }
    for (int e = 0; e < E; ++e) {
        if (experts[e] == nullptr) return false;
        T->ex[e] = experts[e];
        vec = vec && aligned16(experts[e]);
    }
    S->NT = NT, S->M = M, S->mmax = M <= 1 ? 1 : (M <= 4 ? 4 : 8), S->vec = vec;
    return true;
}

// launch_lds raises the dynamic-LDS allowance of the arm it launches (these workgroups may claim more than kLdsDefault)
#define CGC_LAUNCH(KERNEL, MM, ...)                                                             \
    (S.vec ? launch_lds<KERNEL<MM, true>>(grid, dim3(kThreads), smem, st, __VA_ARGS__)          \
           : launch_lds<KERNEL<MM, false>>(grid, dim3(kThreads), smem, st, __VA_ARGS__))

#define CGC_DISPATCH(KERNEL, ...)                                        \
    RECALGO_CHECK(S.mmax == 1   ? CGC_LAUNCH(KERNEL, 1, __VA_ARGS__)     \
                  : S.mmax == 4 ? CGC_LAUNCH(KERNEL, 4, __VA_ARGS__)     \
                                : CGC_LAUNCH(KERNEL, 8, __VA_ARGS__))

}  // namespace

RECALGO_EXPORT int recalgo_cgc_abi_version(void) { return RECALGO_CGC_ABI_VERSION; }

RECALGO_EXPORT int recalgo_cgc_supported(int In, int E, int G, int H, int n_total, int n_max) {
    return limits_ok(In, E, G, H, n_total, n_max) ? 1 : 0;
}

RECALGO_EXPORT int recalgo_cgc_partial_rows(int B, int In, int n_total) {
    (void)In, (void)n_total;        // (one row per workgroup of the persistent backward grid, whatever the row's width)
    const int want = cdiv(B, kRows);
    return want < 1 ? 1 : (want > kBwdGrid ? kBwdGrid : want);
}

RECALGO_EXPORT int recalgo_cgc_fwd(const float* x, int ldx, const float* const* gate_kernels, const int* n_sel, const int* sel,
                                   const float* const* experts, int B, int In, int E, int G, int H, int sum_outputs,
                                   float* const* outs, float* p, recalgo_stream_t stream) {
    CgcTables T;
    CgcShape S;
    RECALGO_REQUIRE(x != nullptr && outs != nullptr && p != nullptr && ldx >= In);
    RECALGO_REQUIRE(cgc_tables(gate_kernels, n_sel, sel, experts, B, In, E, G, H, sum_outputs, &T, &S));
    CgcFwdPtrs O = {};
    for (int m = 0; m < S.M; ++m) {
        RECALGO_REQUIRE(outs[m] != nullptr);
        O.out[m] = outs[m];
        S.vec = S.vec && aligned16(outs[m]);
    }
    const int want = cdiv(B, kRows);
    const dim3 grid(want > kFwdGrid ? kFwdGrid : want);
    const size_t smem = fwd_lds(In, S.NT, S.mmax);
    hipStream_t st = as_stream(stream);
    CGC_DISPATCH(cgc_fwd_kernel, T, O, x, ldx, B, In, E, G, H, S.NT, sum_outputs != 0, p);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_cgc_bwd(const float* x, int ldx, const float* const* gate_kernels, const int* n_sel, const int* sel,
                                   const float* const* experts, const float* p, const float* const* d_outs, int B, int In,
                                   int E, int G, int H, int sum_outputs, int relu_experts, float* const* d_experts, float* dx,
                                   int lddx, float* partials, recalgo_stream_t stream) {
    CgcTables T;
    CgcShape S;
    RECALGO_REQUIRE(x != nullptr && p != nullptr && d_outs != nullptr && partials != nullptr && ldx >= In);
    RECALGO_REQUIRE(dx == nullptr || lddx >= In);
    RECALGO_REQUIRE(cgc_tables(gate_kernels, n_sel, sel, experts, B, In, E, G, H, sum_outputs, &T, &S));
    RECALGO_REQUIRE(!sum_outputs || d_outs[0] != nullptr);
    CgcBwdPtrs P = {};
    for (int m = 0; m < S.M; ++m) {
        P.dout[m] = d_outs[m];
        S.vec = S.vec && aligned16(d_outs[m]);
    }
    for (int e = 0; e < E; ++e) {
        P.dex[e] = d_experts ? d_experts[e] : nullptr;
        S.vec = S.vec && aligned16(P.dex[e]);
    }
    const dim3 grid(recalgo_cgc_partial_rows(B, In, S.NT));
    const size_t smem = bwd_lds(In, S.NT, S.mmax);
    hipStream_t st = as_stream(stream);
    CGC_DISPATCH(cgc_bwd_kernel, T, P, x, ldx, p, B, In, E, G, H, S.NT, sum_outputs != 0, relu_experts, dx, lddx, partials);
    RECALGO_RETURN_LAST();
}
