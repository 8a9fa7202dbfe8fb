// DeepCrossing's residual stack (include/recalgo_res.h), one kernel each way for the WHOLE stack of L units.
//
// A workgroup (512 threads = 8 waves) owns kRows = 32 rows from the first unit to the last: the row tile x_l [32][D] and the
// h_l tile [32][H] live in LDS, nothing but the saved activations goes to memory between the units.  Both products of a
// unit run on v_mfma_f32_16x16x4_f32: the A operand is the LDS tile, the B operand (the weights) is streamed from global
// memory / L2, one dword per lane and k-step (every workgroup reads the same weights: after the first they are L2 hits).
// A wave takes the 16-column tiles wave, wave + 8, .. of the result and keeps kRT = 2 row tiles of it, which share the B
// fragment.  k-step s multiplies k = 4 s .. 4 s + 3 (lane (l16, kq) holds A[row l16][4 s + kq] and B[4 s + kq][column l16]).
// A dot product is kU = 8 k-ordered fmaf chains, step s in chain s % 8, each from 0, added pairwise at the end
// (((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7))): a fixed order, whatever the batch size or the row's place in it, so
// 16 INDEPENDENT accumulators per wave (16x16x4: 32-cycle issue, 40-cycle dependent latency).
//
// Padding to the MFMA tile happens in LDS with zeros: the tiles start as zeros, rows past B are never loaded or stored
// (what the units make of them is dropped), and the columns D .. round4(D) - 1 stay zero; a B-operand load of a column
// past N reads column N - 1 instead (its result is dropped), one of a k past K is replaced by zero.  No load or store
// leaves [B, D] / [B, H] / the weight matrices.
//
// LDS row stride: round4(width) padded to 2 (mod 32) floats: lanes (l16, kq) and (l16, kq + 1) of a 32-lane half then
// read 32 different banks (ds_read_b32 of the A operand is conflict free).  The row tiles are moved between memory and LDS
// by all threads (16-byte global accesses on the VEC arm), never by the MFMA epilogues, which write LDS only.
#include "common.h"

#include "../../include/recalgo_res.h"

namespace {

constexpr int kThreads = 512, kWaves = kThreads / 64;
constexpr int kRows = 32, kRT = kRows / 16;
constexpr int kU = 8;                     // chains of a dot product = k-steps per chunk of tile_gemm's loop
constexpr int kMaxD = RECALGO_RES_MAX_D, kMaxH = RECALGO_RES_MAX_H, kMaxL = RECALGO_RES_MAX_UNITS;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct ResTables {
    const float* w0[kMaxL];
    const float* b0[kMaxL];
    const float* w1[kMaxL];
    const float* b1[kMaxL];
};

__host__ __device__ constexpr int lds_stride(int width) {
    const int w4 = (width + 3) & ~3;
    return w4 + ((34 - (w4 & 31)) & 31);
}
size_t lds_bytes(int D, int H) { return (size_t)kRows * (lds_stride(D) + lds_stride(H)) * sizeof(float); }

// tile [kRows][stride] (LDS) <- src [nb][W] (rows past nb and the padding are left as they are)
template <bool VEC>
__device__ __forceinline__ void tile_load(float* tile, int stride, const float* __restrict__ src, int nb, int W) {
    if (VEC) {
        const int W4 = W >> 2;
        for (int i = threadIdx.x; i < nb * W4; i += kThreads) {
            const int r = i / W4, c = (i - r * W4) * 4;
            const float4 v = *reinterpret_cast<const float4*>(src + (size_t)r * W + c);
            float* t = tile + r * stride + c;
            t[0] = v.x, t[1] = v.y, t[2] = v.z, t[3] = v.w;
        }
    } else {
        for (int i = threadIdx.x; i < nb * W; i += kThreads) {
            const int r = i / W, c = i - r * W;
            tile[r * stride + c] = src[(size_t)r * W + c];
        }
    }
}
template <bool VEC>
__device__ __forceinline__ void tile_store(float* __restrict__ dst, const float* tile, int stride, int nb, int W) {
    if (VEC) {
        const int W4 = W >> 2;
        for (int i = threadIdx.x; i < nb * W4; i += kThreads) {
            const int r = i / W4, c = (i - r * W4) * 4;
            const float* t = tile + r * stride + c;
            *reinterpret_cast<float4*>(dst + (size_t)r * W + c) = make_float4(t[0], t[1], t[2], t[3]);
        }
    } else {
        for (int i = threadIdx.x; i < nb * W; i += kThreads) {
            const int r = i / W, c = i - r * W;
            dst[(size_t)r * W + c] = tile[r * stride + c];
        }
    }
}
// tile <- tile * [mask > 0] (exactly 0.0 under a zero mask), dst <- the masked tile; mask, dst [nb][W]
template <bool VEC>
__device__ __forceinline__ void tile_mask_store(float* tile, int stride, const float* __restrict__ mask, float* __restrict__ dst,
                                                int nb, int W) {
    if (VEC) {
        const int W4 = W >> 2;
        for (int i = threadIdx.x; i < nb * W4; i += kThreads) {
            const int r = i / W4, c = (i - r * W4) * 4;
            const float4 m = *reinterpret_cast<const float4*>(mask + (size_t)r * W + c);
            float* t = tile + r * stride + c;
            const float4 v = make_float4(m.x > 0.f ? t[0] : 0.f, m.y > 0.f ? t[1] : 0.f, m.z > 0.f ? t[2] : 0.f,
                                         m.w > 0.f ? t[3] : 0.f);
            t[0] = v.x, t[1] = v.y, t[2] = v.z, t[3] = v.w;
            *reinterpret_cast<float4*>(dst + (size_t)r * W + c) = v;
        }
    } else {
        for (int i = threadIdx.x; i < nb * W; i += kThreads) {
            const int r = i / W, c = i - r * W;
            const float v = mask[(size_t)r * W + c] > 0.f ? tile[r * stride + c] : 0.f;
            tile[r * stride + c] = v;
            dst[(size_t)r * W + c] = v;
        }
    }
}

// C [kRows][N] = A [kRows][K] (LDS, row stride `as`, zero beyond K up to round4(K)) x Bm, with Bm[k][n] = w[k * ldk + n * ldn]
// (ldk = N, ldn = 1: w is [K, N] row-major; ldk = 1, ldn = K: w is [N, K] row-major, the product with its transpose).
// epi(row, column, value) receives every element of the columns < N once, from the lane that holds it.
template <typename Epi>
__device__ __forceinline__ void tile_gemm(const float* As, int as, int K, int N, const float* __restrict__ w, int ldk, int ldn,
                                          Epi epi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane >> 4, l16 = lane & 15;
    const int NS = (K + 3) >> 2;                          // k-steps; the last one is partial when K % 4 != 0
    for (int ct = wave; ct * 16 < N; ct += kWaves) {
        const int col = ct * 16 + l16;
        const float* bp = w + (size_t)min(col, N - 1) * ldn;
        const float* ap = As + l16 * as + kq;
        // B[4 s + kq][col] of step s; a k past K reads row K - 1 and counts as zero (A is zero there as well)
        auto ldb = [&](int s) {
            const int kk = 4 * s + kq;
            const float v = bp[(size_t)min(kk, K - 1) * ldk];
            return kk < K ? v : 0.f;
        };
        f32x4 acc[kU][kRT];
#pragma unroll
        for (int u = 0; u < kU; ++u)
#pragma unroll
            for (int t = 0; t < kRT; ++t) acc[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        // chunks of kU k-steps, step s into chain s % kU; the B loads of the next chunk are in flight under the MFMAs of
        // this one
        float b[kU], bn[kU] = {};
#pragma unroll
        for (int u = 0; u < kU; ++u) b[u] = ldb(u);
        for (int s0 = 0; s0 < NS; s0 += kU) {
            if (s0 + kU < NS) {
#pragma unroll
                for (int u = 0; u < kU; ++u) bn[u] = ldb(s0 + kU + u);
            }
            if (s0 + kU <= NS) {
#pragma unroll
                for (int u = 0; u < kU; ++u)
#pragma unroll
                    for (int t = 0; t < kRT; ++t)
                        acc[u][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[t * 16 * as + 4 * (s0 + u)], b[u], acc[u][t], 0, 0, 0);
            } else {                                      // the last chunk of a K that is no multiple of 4 kU
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    if (s0 + u < NS) {
#pragma unroll
                        for (int t = 0; t < kRT; ++t)
                            acc[u][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[t * 16 * as + 4 * (s0 + u)], b[u], acc[u][t], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) b[u] = bn[u];
        }
        // the chains, added pairwise: ((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7))
#pragma unroll
        for (int st = 1; st < kU; st *= 2)
#pragma unroll
            for (int u = 0; u < kU; u += 2 * st)
#pragma unroll
                for (int t = 0; t < kRT; ++t) acc[u][t] += acc[u + st][t];
        // accumulator register r of lane (l16, kq): row 4 kq + r, column l16 of the 16 x 16 tile
        if (col < N) {
#pragma unroll
            for (int t = 0; t < kRT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) epi(t * 16 + 4 * kq + r, col, acc[0][t][r]);
        }
    }
}

__device__ __forceinline__ void zero_lds(float* smem, int floats) {
    for (int i = threadIdx.x; i < floats; i += kThreads) smem[i] = 0.f;
    __syncthreads();
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void res_stack_fwd_kernel(const float* __restrict__ x, ResTables T, int B, int D, int H,
                                                                 int L, int save, float* __restrict__ hs,
                                                                 float* __restrict__ ys) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int XS = lds_stride(D), HS = lds_stride(H);
    float* Xs = smem;                                     // [kRows][XS]  x_l, then x_{l+1} in place
    float* Hs = smem + kRows * XS;                        // [kRows][HS]  h_l
    const int b0 = blockIdx.x * kRows, nb = min(kRows, B - b0);
    zero_lds(smem, kRows * (XS + HS));
    tile_load<VEC>(Xs, XS, x + (size_t)b0 * D, nb, D);
    __syncthreads();
    for (int l = 0; l < L; ++l) {
        const float* bias0 = T.b0[l];
        tile_gemm(Xs, XS, D, H, T.w0[l], H, 1, [&](int r, int c, float v) { Hs[r * HS + c] = fmaxf(v + bias0[c], 0.f); });
        __syncthreads();
        if (save) tile_store<VEC>(hs + ((size_t)l * B + b0) * H, Hs, HS, nb, H);
        const float* bias1 = T.b1[l];
        // (each element of Xs is read and rewritten by the one lane that owns it; the product reads Hs only)
        tile_gemm(Hs, HS, H, D, T.w1[l], D, 1, [&](int r, int c, float v) {
            Xs[r * XS + c] = fmaxf(Xs[r * XS + c] + (v + bias1[c]), 0.f);
        });
        __syncthreads();
        if (save) tile_store<VEC>(ys + ((size_t)l * B + b0) * D, Xs, XS, nb, D);
        else if (l == L - 1) tile_store<VEC>(ys + (size_t)b0 * D, Xs, XS, nb, D);
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void res_stack_bwd_kernel(const float* __restrict__ g, const float* __restrict__ hs,
                                                                 const float* __restrict__ ys, ResTables T, int B, int D, int H,
                                                                 int L, float* __restrict__ dzs, float* __restrict__ dhs,
                                                                 float* __restrict__ dx) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int GS = lds_stride(D), HS = lds_stride(H);
    float* Gs = smem;                                     // [kRows][GS]  g_{l+1}, dz_l, then g_l in place
    float* Hs = smem + kRows * GS;                        // [kRows][HS]  dh_l
    const int b0 = blockIdx.x * kRows, nb = min(kRows, B - b0);
    zero_lds(smem, kRows * (GS + HS));
    tile_load<VEC>(Gs, GS, g + (size_t)b0 * D, nb, D);
    __syncthreads();
    for (int l = L - 1; l >= 0; --l) {
        const size_t rowD = ((size_t)l * B + b0) * D, rowH = ((size_t)l * B + b0) * H;
        tile_mask_store<VEC>(Gs, GS, ys + rowD, dzs + rowD, nb, D);                   // dz_l
        __syncthreads();
        tile_gemm(Gs, GS, D, H, T.w1[l], 1, D, [&](int r, int c, float v) { Hs[r * HS + c] = v; });
        __syncthreads();
        tile_mask_store<VEC>(Hs, HS, hs + rowH, dhs + rowH, nb, H);                   // dh_l
        __syncthreads();
        tile_gemm(Hs, HS, H, D, T.w0[l], 1, H, [&](int r, int c, float v) { Gs[r * GS + c] += v; });      // g_l
        __syncthreads();
    }
    tile_store<VEC>(dx + (size_t)b0 * D, Gs, GS, nb, D);
}

bool supported(int D, int H, int L) {
    return D >= 1 && D <= kMaxD && H >= 16 && H <= kMaxH && (H & 15) == 0 && L >= 1 && L <= kMaxL && lds_bytes(D, H) <= kLdsMax;
}

// copies a HOST table of L device pointers; false when one of them is NULL or not 4-byte aligned
bool take_table(const float* const* src, int L, const float** dst) {
    if (src == nullptr) return false;
    for (int l = 0; l < kMaxL; ++l) {
        dst[l] = l < L ? src[l] : nullptr;
        if (l < L && (dst[l] == nullptr || !aligned_to<4>(dst[l]))) return false;
    }
    return true;
}

}  // namespace

RECALGO_EXPORT int recalgo_res_abi_version(void) { return RECALGO_RES_ABI_VERSION; }

RECALGO_EXPORT int recalgo_res_supported(int D, int H, int L) { return supported(D, H, L) ? 1 : 0; }

RECALGO_EXPORT int recalgo_res_stack_fwd(const float* x, const float* const* w0, const float* const* b0, const float* const* w1,
                                         const float* const* b1, int B, int D, int H, int L, int save, float* hs, float* ys,
                                         recalgo_stream_t stream) {
    RECALGO_REQUIRE(supported(D, H, L) && B >= 1);
    RECALGO_REQUIRE(x != nullptr && ys != nullptr && (save == 0 || hs != nullptr) && aligned_to<4>(x, hs, ys));
    ResTables T;
    RECALGO_REQUIRE(take_table(w0, L, T.w0) && take_table(b0, L, T.b0) && take_table(w1, L, T.w1) && take_table(b1, L, T.b1));
    const dim3 grid(cdiv(B, kRows)), block(kThreads);
    const size_t lds = lds_bytes(D, H);
    if ((D & 3) == 0 && aligned16(x, hs, ys))
        RECALGO_CHECK(launch_lds<res_stack_fwd_kernel<true>>(grid, block, lds, as_stream(stream), x, T, B, D, H, L, save, hs, ys));
    else
        RECALGO_CHECK(launch_lds<res_stack_fwd_kernel<false>>(grid, block, lds, as_stream(stream), x, T, B, D, H, L, save, hs, ys));
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_res_stack_bwd(const float* g, const float* hs, const float* ys, const float* const* w0,
                                         const float* const* w1, int B, int D, int H, int L, float* dzs, float* dhs, float* dx,
                                         recalgo_stream_t stream) {
    RECALGO_REQUIRE(supported(D, H, L) && B >= 1);
    RECALGO_REQUIRE(g != nullptr && hs != nullptr && ys != nullptr && dzs != nullptr && dhs != nullptr && dx != nullptr);
    RECALGO_REQUIRE(aligned_to<4>(g, hs, ys, dzs, dhs, dx));
    ResTables T;
    RECALGO_REQUIRE(take_table(w0, L, T.w0) && take_table(w1, L, T.w1));
    for (int l = 0; l < kMaxL; ++l) T.b0[l] = T.b1[l] = nullptr;
    const dim3 grid(cdiv(B, kRows)), block(kThreads);
    const size_t lds = lds_bytes(D, H);
    if ((D & 3) == 0 && aligned16(g, hs, ys, dzs, dhs, dx))
        RECALGO_CHECK(launch_lds<res_stack_bwd_kernel<true>>(grid, block, lds, as_stream(stream), g, hs, ys, T, B, D, H, L, dzs, dhs, dx));
    else
        RECALGO_CHECK(launch_lds<res_stack_bwd_kernel<false>>(grid, block, lds, as_stream(stream), g, hs, ys, T, B, D, H, L, dzs, dhs, dx));
    RECALGO_RETURN_LAST();
}
