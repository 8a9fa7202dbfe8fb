// Multi-gate mixture of experts (MMoE, algorithm/MMOE/mmoe.py:208-232; PLE's CGC block, algorithm/PLE/extraction_network.py,
// is the same block only within this kernel's limits — E, n_g <= 16, 16 KiB of gate kernels; PLE's default sizes are served
// by csrc/cgc.hip): the bias-free softmax gates and the mix of the expert outputs in ONE streaming kernel each way, and the
// T-task sigmoid cross-entropy tail in one launch.
//
//   z_g = x Wg                     x [B, In], Wg [In, n_g]: the gate kernels sit in LDS
//   p_g = softmax(z_g)             max-subtracted
//   out_g[b, :] = sum_j p_g[b, j] * expert_{sel[g][j]}[b, :]
//
// backward, with c[g][e] = sum_{j: sel[g][j] = e} p_g[j]:
//   d_expert_e = sum_g c[g][e] * d_out_g          (zeroed where expert_e <= 0 when the experts are ReLU outputs)
//   dp_g[j]    = <d_out_g, expert_{sel[g][j]}>
//   dz_g       = p_g * (dp_g - sum_j p_g[j] dp_g[j])
//   dx         = sum_g dz_g Wg^T
//   dWg        = x^T dz_g           per-workgroup partials (added in row order inside the workgroup), summed over the
//                                   workgroups in a fixed order by the step's deferred column sums — no float atomics
//
// Shape of both kernels: one wave64 per example row, four rows per 256-thread workgroup, 16-byte loads and stores along H
// (each lane holds the E expert vectors of its H-chunk in registers, every gate reuses them), no MFMA.  The mix itself is
// evaluated in its dense form over c[g][e], so a PLE-style selection costs G * E multiply-adds per element instead of
// sum n_g — still far below the load / store time of the element.
//
// Arms: EMAX in {4, 8, 16} >= max(E, G) bounds the register arrays (compile-time indices only); VEC = every expert, output
// and gradient base pointer is 16-byte aligned (float4 accesses), else the same kernels with four scalar accesses per chunk.
#include "common.h"
#include "sigmoid_ce.h"

namespace {

constexpr int kMixMax = RECALGO_GATE_MIX_MAX;          // E, G, n_g
constexpr int kMixMaxIn = 512;                         // 8 x-slots per lane
constexpr int kMixWFloats = 4096;                      // LDS budget of the staged gate kernels: In * (NT | 1) floats (16 KiB)
constexpr int kMixRows = 4;                            // rows (= waves) per workgroup

struct MixTables {
    const float* wg[kMixMax];
    const float* ex[kMixMax];
    int n[kMixMax];
    int off[kMixMax];
    uint64_t sel[kMixMax];          // 4 bits per position
};
struct MixFwdPtrs {
    float* out[kMixMax];
};
struct MixBwdPtrs {
    const float* dout[kMixMax];
    float* dex[kMixMax];
};

// gate kernels -> Ws[k * ldw + off_g + j], the tables -> tab = [n[16] | off[16] | sel[16 * 16]]
__device__ __forceinline__ void stage_gates(const MixTables& T, int In, int G, int ldw, float* Ws, int* tab) {
    for (int g = 0; g < G; ++g) {
        const float* w = T.wg[g];
        const int n = T.n[g], off = T.off[g];
        for (int i = threadIdx.x; i < In * n; i += 256) {
            const int k = i / n, j = i - k * n;
            Ws[k * ldw + off + j] = w[i];
        }
        if (threadIdx.x < kMixMax) tab[2 * kMixMax + g * kMixMax + threadIdx.x] = (int)((T.sel[g] >> (4 * threadIdx.x)) & 15);
        if (threadIdx.x == 0) tab[g] = n, tab[kMixMax + g] = off;
    }
}

// cs[g * EMAX + e] = sum of the gate's probabilities that select expert e (ps: the row's probabilities)
template <int EMAX>
__device__ __forceinline__ void mix_coefficients(const int* tab, const float* ps, float* cs, int G, int lane) {
    for (int i = lane; i < G * EMAX; i += 64) cs[i] = 0.f;
    wave_sync();
    if (lane < G) {
        const int n = tab[lane], off = tab[kMixMax + lane];
        const int* sel = tab + 2 * kMixMax + lane * kMixMax;
        for (int j = 0; j < n; ++j) cs[lane * EMAX + sel[j]] += ps[off + j];
    }
    wave_sync();
}

template <int EMAX, bool VEC>
__global__ __launch_bounds__(256) void gate_mix_fwd_kernel(MixTables T, MixFwdPtrs O, const float* __restrict__ x, int ldx,
                                                           int B, int In, int E, int G, int H, int NT,
                                                           float* __restrict__ p_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int ldw = NT | 1, NT4 = round4(NT);
    float* Ws = reinterpret_cast<float*>(smem);
    int* tab = reinterpret_cast<int*>(Ws + round4(In * ldw));
    float* wave_s = reinterpret_cast<float*>(tab + 2 * kMixMax + kMixMax * kMixMax);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* zs = reinterpret_cast<double*>(wave_s + wave * (3 * NT4 + kMixMax * EMAX));
    float* ps = reinterpret_cast<float*>(zs + NT4);
    float* cs = ps + NT4;
    stage_gates(T, In, G, ldw, Ws, tab);
    __syncthreads();
    const int H4 = H >> 2;
    for (int row = blockIdx.x * kMixRows + wave; row < B; row += gridDim.x * kMixRows) {
        // z = x Wg: the lanes split In, one wave sum per gate column.  The gate logits and their softmax are NT numbers per
        // row: they are evaluated in double (a logit of magnitude 80 carries 4e-6 of rounding per fp32 operation, which the
        // softmax turns into that much RELATIVE error of every probability and of everything the backward derives from them)
        float xk[kMixMaxIn / 64];
        int kk[kMixMaxIn / 64];
#pragma unroll
        for (int i = 0; i < kMixMaxIn / 64; ++i) {
            const int k = lane + 64 * i;
            kk[i] = (k < In ? k : In - 1) * ldw;
            xk[i] = (64 * i < In && k < In) ? x[(size_t)row * ldx + k] : 0.f;
        }
        for (int c = 0; c < NT; ++c) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < kMixMaxIn / 64; ++i)
                if (64 * i < In) s = fma((double)xk[i], (double)Ws[kk[i] + c], s);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) zs[c] = s;
        }
        wave_sync();
        if (lane < G) {          // softmax of gate `lane` (n_g <= 16 terms)
            const int n = tab[lane], off = tab[kMixMax + lane];
            double m = zs[off];
            for (int j = 1; j < n; ++j) m = fmax(m, zs[off + j]);
            double sum = 0.0;
            for (int j = 0; j < n; ++j) {
                const double e = exp(zs[off + j] - m);
                zs[off + j] = e;
                sum += e;
            }
            for (int j = 0; j < n; ++j) {
                const float p = (float)(zs[off + j] / sum);
                ps[off + j] = p;
                p_out[(size_t)row * NT + off + j] = p;
            }
        }
        wave_sync();
        mix_coefficients<EMAX>(tab, ps, cs, G, lane);
        for (int i = lane; i < H4; i += 64) {
            const size_t at = (size_t)row * H + 4 * i;
            float4 ev[EMAX];
#pragma unroll
            for (int e = 0; e < EMAX; ++e)
                if (e < E) ev[e] = ld4<VEC>(T.ex[e] + at);
            for (int g = 0; g < G; ++g) {
                float4 acc = f4_zero();
#pragma unroll
                for (int e = 0; e < EMAX; ++e)
                    if (e < E) acc = f4_fma(ev[e], cs[g * EMAX + e], acc);
                st4<VEC>(O.out[g] + at, acc);
            }
        }
        wave_sync();             // (the next row overwrites ps / cs)
    }
}

template <int EMAX, bool VEC>
__global__ __launch_bounds__(256) void gate_mix_bwd_kernel(MixTables T, MixBwdPtrs P, const float* __restrict__ x, int ldx,
                                                           const float* __restrict__ p_in, int B, int In, int E, int G, int H,
                                                           int NT, int relu_experts, float* __restrict__ dx, int lddx,
                                                           float* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int ldw = NT | 1, NT4 = round4(NT), W4 = round4(In * ldw), In4 = round4(In);
    float* Ws = reinterpret_cast<float*>(smem);
    float* dWs = Ws + W4;
    int* tab = reinterpret_cast<int*>(dWs + W4);
    float* wave_s = reinterpret_cast<float*>(tab + 2 * kMixMax + kMixMax * kMixMax);
    const int per_wave = 2 * NT4 + 2 * kMixMax * EMAX + In4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* ps = wave_s + wave * per_wave;
    float* dzs = ps + NT4;
    float* cs = dzs + NT4;
    float* dpe = cs + kMixMax * EMAX;
    float* xs = dpe + kMixMax * EMAX;
    stage_gates(T, In, G, ldw, Ws, tab);
    for (int i = threadIdx.x; i < W4; i += 256) dWs[i] = 0.f;
    __syncthreads();
    const int H4 = H >> 2;
    const int rounds = (B + gridDim.x * kMixRows - 1) / (gridDim.x * kMixRows);
    for (int r = 0; r < rounds; ++r) {
        const int row = (r * gridDim.x + blockIdx.x) * kMixRows + wave;
        const bool valid = row < B;                      // (wave-uniform; a wave without a row adds exact zeros to dWg)
        for (int i = lane; i < NT; i += 64) {
            ps[i] = valid ? p_in[(size_t)row * NT + i] : 0.f;
            dzs[i] = 0.f;
        }
        for (int i = lane; i < In; i += 64) xs[i] = valid ? x[(size_t)row * ldx + i] : 0.f;
        mix_coefficients<EMAX>(tab, ps, cs, G, lane);
        if (valid) {
            float acc[EMAX][EMAX];                       // [g][e]: this lane's share of <d_out_g, expert_e>
#pragma unroll
            for (int g = 0; g < EMAX; ++g)
#pragma unroll
                for (int e = 0; e < EMAX; ++e) acc[g][e] = 0.f;
            for (int i = lane; i < H4; i += 64) {
                const size_t at = (size_t)row * H + 4 * i;
                float4 ev[EMAX], de[EMAX];
#pragma unroll
                for (int e = 0; e < EMAX; ++e) {
                    if (e < E) ev[e] = ld4<VEC>(T.ex[e] + at);
                    de[e] = f4_zero();
                }
#pragma unroll
                for (int g = 0; g < EMAX; ++g) {
                    if (g < G && P.dout[g] != nullptr) {
                        const float4 dg = ld4<VEC>(P.dout[g] + at);
#pragma unroll
                        for (int e = 0; e < EMAX; ++e) {
                            if (e < E) {
                                acc[g][e] += f4_dot(dg, ev[e]);
                                de[e] = f4_fma(dg, cs[g * EMAX + e], de[e]);
                            }
                        }
                    }
                }
#pragma unroll
                for (int e = 0; e < EMAX; ++e) {
                    if (e < E && P.dex[e] != nullptr) {
                        float4 v = de[e];
                        if (relu_experts) {
                            v.x = ev[e].x > 0.f ? v.x : 0.f, v.y = ev[e].y > 0.f ? v.y : 0.f;
                            v.z = ev[e].z > 0.f ? v.z : 0.f, v.w = ev[e].w > 0.f ? v.w : 0.f;
                        }
                        st4<VEC>(P.dex[e] + at, v);
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < EMAX; ++g) {
#pragma unroll
                for (int e = 0; e < EMAX; ++e) {
                    if (g < G && e < E) {
                        const float v = wave_sum(acc[g][e]);
                        if (lane == 0) dpe[g * EMAX + e] = v;
                    }
                }
            }
            wave_sync();
            if (lane < G) {      // dz of gate `lane`
                const int n = tab[lane], off = tab[kMixMax + lane];
                const int* sel = tab + 2 * kMixMax + lane * kMixMax;
                float s = 0.f;
                for (int j = 0; j < n; ++j) s = fmaf(ps[off + j], dpe[lane * EMAX + sel[j]], s);
                for (int j = 0; j < n; ++j) dzs[off + j] = ps[off + j] * (dpe[lane * EMAX + sel[j]] - s);
            }
            wave_sync();
            if (dx != nullptr) {
                for (int k = lane; k < In; k += 64) {
                    float s = 0.f;
                    for (int c = 0; c < NT; ++c) s = fmaf(dzs[c], Ws[k * ldw + c], s);
                    dx[(size_t)row * lddx + k] = s;
                }
            }
        }
        __syncthreads();
        // dWg += x^T dz over the workgroup's four rows, in row order
        for (int idx = threadIdx.x; idx < In * NT; idx += 256) {
            const int k = idx / NT, c = idx - k * NT;
            float a = dWs[k * ldw + c];
#pragma unroll
            for (int w = 0; w < kMixRows; ++w) a = fmaf(wave_s[w * per_wave + 2 * NT4 + 2 * kMixMax * EMAX + k], wave_s[w * per_wave + NT4 + c], a);
            dWs[k * ldw + c] = a;
        }
        __syncthreads();
    }
    // partials[block][In * off_g + k * n_g + j]: gate g's [In, n_g] kernel gradient is one contiguous run of the row
    float* prow = partials + (size_t)blockIdx.x * In * NT;
    for (int g = 0; g < G; ++g) {
        const int n = tab[g], off = tab[kMixMax + g];
        for (int i = threadIdx.x; i < In * n; i += 256) {
            const int k = i / n, j = i - k * n;
            prow[In * off + i] = dWs[k * ldw + off + j];
        }
    }
}

// The loss tail of T tasks in one launch: one 1024-thread workgroup walks the tasks in order, each through sigmoid_ce_task
// (sigmoid_ce.h) — the device function sigmoid_ce_kernel (csrc/tail.hip) is made of, so a task's value is that kernel's
// bit for bit.  T * B elements pass through the one workgroup
// task after task: 19.5 us at T = 3, B = 4096 (2 % of the MMoE step); many tasks or a much larger B want a grid over tasks.
struct TaskPtrs {
    const float* logits[kMixMax];
    const float* labels[kMixMax];
};

__global__ __launch_bounds__(1024) void multitask_sigmoid_ce_kernel(TaskPtrs P, unsigned T, unsigned B, float grad_scale,
                                                                    float* __restrict__ prob, float* __restrict__ losses,
                                                                    float* __restrict__ total, float* __restrict__ dlogit) {
    __shared__ float red[16];
    float sum = 0.f;
    for (unsigned t = 0; t < T; ++t) {
        const float l = sigmoid_ce_task(
            P.logits[t], P.labels[t], B, grad_scale, dlogit != nullptr, red,
            [&](unsigned i, float p) { prob[(size_t)i * T + t] = p; },
            [&](unsigned i, float d) { dlogit[(size_t)t * B + i] = d; });
        if (threadIdx.x == 0) {
            losses[t] = l;
            sum = t == 0 ? l : sum + l;                  // tf.add_n: left to right
        }
        __syncthreads();                                 // (`red` is reused by the next task)
    }
    if (threadIdx.x == 0) total[0] = sum;
}

struct MixShape {
    int NT, emax;
    bool vec;
};

// validates the tables and fills T; -> false outside the served limits
bool mix_tables(const float* const* gate_kernels, const int* n_sel, const int* sel, const float* const* experts, int B, int In,
                int E, int G, int H, MixTables* T, MixShape* S) {
    if (!gate_kernels || !n_sel || !sel || !experts || B < 1 || In < 1 || In > kMixMaxIn || E < 1 || E > kMixMax || G < 1 ||
        G > kMixMax || H < 4 || (H & 3))
        return false;
    int NT = 0;
    bool vec = true;
    for (int g = 0; g < kMixMax; ++g) {
        T->wg[g] = nullptr, T->n[g] = 0, T->off[g] = 0;
        T->sel[g] = 0;
    }
    for (int e = 0; e < kMixMax; ++e) T->ex[e] = nullptr;
    for (int g = 0; g < G; ++g) {
        const int n = n_sel[g];
        if (n < 1 || n > kMixMax || gate_kernels[g] == nullptr) return false;
        T->wg[g] = gate_kernels[g], T->n[g] = n, T->off[g] = NT;
        for (int j = 0; j < n; ++j) {
            if (sel[NT + j] < 0 || sel[NT + j] >= E) return false;
            T->sel[g] |= (uint64_t)sel[NT + j] << (4 * j);
        }
        NT += n;
    }
    if ((int64_t)In * (NT | 1) > kMixWFloats) return false;
    for (int e = 0; e < E; ++e) {
        if (experts[e] == nullptr) return false;
        T->ex[e] = experts[e];
        vec = vec && aligned16(experts[e]);
    }
    const int m = E > G ? E : G;
    S->NT = NT, S->emax = m <= 4 ? 4 : (m <= 8 ? 8 : 16), S->vec = vec;
    return true;
}

}  // namespace

RECALGO_EXPORT int recalgo_gate_mix_supported(int In, int E, int G, int H, int n_total) {
    return In >= 1 && In <= kMixMaxIn && E >= 1 && E <= kMixMax && G >= 1 && G <= kMixMax && H >= 4 && (H & 3) == 0 &&
           n_total >= G && n_total <= kMixMax * kMixMax && (int64_t)In * (n_total | 1) <= kMixWFloats;
}

RECALGO_EXPORT int recalgo_gate_mix_partial_rows(int B) {
    const int want = cdiv(B, kMixRows);
    return want < 1 ? 1 : (want > 1024 ? 1024 : want);
}

#define MIX_DISPATCH(KERNEL, ...)                                                                        \
    do {                                                                                                 \
        if (S.emax == 4) {                                                                               \
            if (S.vec) hipLaunchKernelGGL((KERNEL<4, true>), grid, dim3(256), smem, st, __VA_ARGS__);    \
            else hipLaunchKernelGGL((KERNEL<4, false>), grid, dim3(256), smem, st, __VA_ARGS__);         \
        } else if (S.emax == 8) {                                                                        \
            if (S.vec) hipLaunchKernelGGL((KERNEL<8, true>), grid, dim3(256), smem, st, __VA_ARGS__);    \
            else hipLaunchKernelGGL((KERNEL<8, false>), grid, dim3(256), smem, st, __VA_ARGS__);         \
        } else {                                                                                         \
            if (S.vec) hipLaunchKernelGGL((KERNEL<16, true>), grid, dim3(256), smem, st, __VA_ARGS__);   \
            else hipLaunchKernelGGL((KERNEL<16, false>), grid, dim3(256), smem, st, __VA_ARGS__);        \
        }                                                                                                \
    } while (0)

RECALGO_EXPORT int recalgo_gate_mix_fwd(const float* x, int ldx, const float* const* gate_kernels, const int* n_sel,
                                        const int* sel, const float* const* experts, int B, int In, int E, int G, int H,
                                        float* const* outs, float* p, recalgo_stream_t stream) {
    MixTables T;
    MixShape S;
    RECALGO_REQUIRE(x != nullptr && outs != nullptr && p != nullptr && ldx >= In);
    RECALGO_REQUIRE(mix_tables(gate_kernels, n_sel, sel, experts, B, In, E, G, H, &T, &S));
    MixFwdPtrs O;
    for (int g = 0; g < kMixMax; ++g) {
        O.out[g] = g < G ? outs[g] : nullptr;
        if (g < G) {
            RECALGO_REQUIRE(outs[g] != nullptr);
            S.vec = S.vec && aligned16(outs[g]);
        }
    }
    const int want = cdiv(B, kMixRows);
    const dim3 grid(want > 4096 ? 4096 : want);
    const size_t smem = sizeof(float) * (round4(In * (S.NT | 1)) + 2 * kMixMax + kMixMax * kMixMax +
                                         kMixRows * (3 * round4(S.NT) + kMixMax * S.emax));
    hipStream_t st = as_stream(stream);
    MIX_DISPATCH(gate_mix_fwd_kernel, T, O, x, ldx, B, In, E, G, H, S.NT, p);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_gate_mix_bwd(const float* x, int ldx, const float* const* gate_kernels, const int* n_sel,
                                        const int* sel, const float* const* experts, const float* p,
                                        const float* const* d_outs, int B, int In, int E, int G, int H, int relu_experts,
                                        float* const* d_experts, float* dx, int lddx, float* partials,
                                        recalgo_stream_t stream) {
    MixTables T;
    MixShape S;
    RECALGO_REQUIRE(x != nullptr && p != nullptr && d_outs != nullptr && partials != nullptr && ldx >= In);
    RECALGO_REQUIRE(dx == nullptr || lddx >= In);
    RECALGO_REQUIRE(mix_tables(gate_kernels, n_sel, sel, experts, B, In, E, G, H, &T, &S));
    MixBwdPtrs P;
    for (int i = 0; i < kMixMax; ++i) {
        P.dout[i] = i < G ? d_outs[i] : nullptr;
        P.dex[i] = (i < E && d_experts) ? d_experts[i] : nullptr;
        S.vec = S.vec && aligned16(P.dout[i], P.dex[i]);
    }
    const dim3 grid(recalgo_gate_mix_partial_rows(B));
    const size_t smem = sizeof(float) * (2 * round4(In * (S.NT | 1)) + 2 * kMixMax + kMixMax * kMixMax +
                                         kMixRows * (2 * round4(S.NT) + 2 * kMixMax * S.emax + round4(In)));
    hipStream_t st = as_stream(stream);
    MIX_DISPATCH(gate_mix_bwd_kernel, T, P, x, ldx, p, B, In, E, G, H, S.NT, relu_experts, dx, lddx, partials);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_multitask_sigmoid_ce_fwd_bwd(const float* const* logits, const float* const* labels, int T, int B,
                                                        float grad_scale, float* prob, float* losses, float* total,
                                                        float* dlogit, recalgo_stream_t stream) {
    RECALGO_REQUIRE(logits != nullptr && labels != nullptr && T >= 1 && T <= kMixMax && B > 0 && prob != nullptr &&
                    losses != nullptr && total != nullptr);
    TaskPtrs P;
    for (int t = 0; t < kMixMax; ++t) {
        P.logits[t] = t < T ? logits[t] : nullptr;
        P.labels[t] = t < T ? labels[t] : nullptr;
        if (t < T) RECALGO_REQUIRE(logits[t] != nullptr && labels[t] != nullptr);
    }
    hipLaunchKernelGGL(multitask_sigmoid_ce_kernel, dim3(1), dim3(1024), 0, as_stream(stream), P, (unsigned)T, (unsigned)B,
                       grad_scale, prob, losses, total, dlogit);
    RECALGO_RETURN_LAST();
}
