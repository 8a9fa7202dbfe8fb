// The hidden MLP tower of a small serving request in ONE launch (include/recalgo_serve.h): up to four layers of
//     h <- fmaf(relu(h W + b), scale, shift)          (dense(relu) -> [dropout = identity] -> [BatchNorm inference, folded])
// Per layer the serving path otherwise launches the dense engine and, with a BatchNorm, the elementwise scale / shift: each of
// them a launch's fixed cost and a round trip of the activations through L2.  Here the activations never leave the workgroup.
// Measured (profiles/serving_bench.json, 416 -> 512 -> 256 -> 128): ~51 us at every B from 1 to 4096, against 67 .. 98 us for three
// dense + three BatchNorm launches and 35 .. 47 us for three dense launches alone — it pays where a BatchNorm is folded.  Built after csrc/tailfuse.hip, as a latency chain rather than a throughput kernel:
//   * 16 rows per workgroup, 8 waves, v_mfma_f32_16x16x4_f32; wave w owns the 16-column tiles w, w + 8, .. of a layer (at most
//     four: 512 columns), all of them in flight together: 2 accumulator chains per tile, so a wave with one tile still has two
//     independent MFMAs (a dependent 16x16x4 issues every 40 cycles, not 32);
//   * the activation tile of the current and of the next layer ping-pong between two LDS buffers (A operand: one ds_read_b128
//     per four steps; up to 16 x 1024 + 16 x 512 floats, more than 64 KiB: launch_lds owns the opt-in), rows past B and columns
//     past K zero-filled, so no step of the main loop is conditional;
//   * the B operand comes straight from global memory / L2 into registers, one chunk of k ahead of the MFMAs that use it (a
//     wave with fewer tiles runs longer chunks: the same number of loads in flight); the first chunk of the NEXT layer is
//     requested before the current layer's epilogue, so it crosses the barrier between two layers in flight;
//   * plain vector stores only; the last layer's epilogue writes `out`, masked to the rows that exist.
#include "common.h"
#include "../../include/recalgo_serve.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kRows = 16;                // rows per workgroup
constexpr int kThreads = 512, kWaves = 8;
constexpr int kMaxL = RECALGO_SERVE_MAX_LAYERS;
constexpr int kPadK = 128;               // an LDS tile is zero-filled up to the next multiple of this many columns (the longest chunk)
constexpr int kMaxTiles = 4;             // column tiles of one wave: 512 / 16 / 8
constexpr int kChunkRegs = 32;           // B-operand registers of one chunk: tiles x groups x 4

struct TowerArgs {
    const float* x;
    float* out;
    const float* w[kMaxL];
    const float* b[kMaxL];
    const float* scale[kMaxL];
    const float* shift[kMaxL];
    int units[kMaxL];
    int L;
    unsigned relu_bits;
    int B, K0;
    int stride0, stride1;                // row strides of the two LDS buffers (floats; % 4 == 0, and % 128 == 4: conflict-free b128 reads)
    int vec_x;                           // x moves as float4
};

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float f4_at(const float4& v, int x) { return x == 0 ? v.x : (x == 1 ? v.y : (x == 2 ? v.z : v.w)); }

__host__ __device__ __forceinline__ int pad_k(int k) { return (k + kPadK - 1) / kPadK * kPadK; }
// tiles of wave `wave` in a layer of N columns
__device__ __forceinline__ int tiles_of(int N, unsigned wave) {
    const int tiles = N / 16;
    return tiles > (int)wave ? (tiles - (int)wave + kWaves - 1) / kWaves : 0;
}

// Chunk `chunk` (CG groups of 16 k) of the B operand of this wave's NT tiles: step x of group j of tile t multiplies
// k = 16 (chunk CG + j) + 4 kq + x.  Rows past K are never read (the address is clamped) and count as exact zeros.
template <int NT, int CG>
__device__ __forceinline__ void load_chunk(float (&bq)[kChunkRegs], const float* __restrict__ W, int K, int N, int chunk,
                                           unsigned wave, unsigned l16, unsigned kq) {
    static_assert(NT * CG * 4 <= kChunkRegs, "chunk registers");
#pragma unroll
    for (int j = 0; j < CG; ++j)
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int k = 16 * (chunk * CG + j) + 4 * (int)kq + x;
            const float* row = W + (size_t)min(k, K - 1) * N + l16;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float v = row[(wave + kWaves * t) * 16];
                bq[(t * CG + j) * 4 + x] = k < K ? v : 0.f;
            }
        }
}

template <int NT, int CG>
__device__ __forceinline__ void run_layer(const float* __restrict__ A, int stride, const float* __restrict__ W,
                                          const float* __restrict__ bias, int K, int N, float (&bq)[kChunkRegs],
                                          f32x4 (&acc)[kMaxTiles], unsigned wave, unsigned l16, unsigned kq) {
    static_assert(CG % 2 == 0, "a group's chain is its parity inside the chunk");
    f32x4 c0[NT], c1[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const float b = bias ? bias[(wave + kWaves * t) * 16 + l16] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) { c0[t][r] = b; c1[t][r] = 0.f; }
    }
    const int nchunks = (K + 16 * CG - 1) / (16 * CG);
    const float* arow = A + l16 * stride + 4 * kq;
    for (int c = 0; c < nchunks; ++c) {
        float nxt[kChunkRegs];
        if (c + 1 < nchunks) load_chunk<NT, CG>(nxt, W, K, N, c + 1, wave, l16, kq);
#pragma unroll
        for (int j = 0; j < CG; ++j) {
            const float4 a = *reinterpret_cast<const float4*>(arow + 16 * (c * CG + j));
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if (j & 1) c1[t] = mfma16(f4_at(a, x), bq[(t * CG + j) * 4 + x], c1[t]);
                    else c0[t] = mfma16(f4_at(a, x), bq[(t * CG + j) * 4 + x], c0[t]);
                }
        }
        if (c + 1 < nchunks) {
#pragma unroll
            for (int i = 0; i < NT * CG * 4; ++i) bq[i] = nxt[i];
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] = c0[t][r] + c1[t][r];
}

// the chunk length of a wave with nt tiles: the same number of B loads in flight whatever the layer's width
#define SERVE_BY_TILES(nt, CALL)          \
    switch (nt) {                         \
        case 1: { CALL(1, 8); break; }    \
        case 2: { CALL(2, 4); break; }    \
        case 3: { CALL(3, 2); break; }    \
        case 4: { CALL(4, 2); break; }    \
        default: break;                   \
    }

__global__ __launch_bounds__(kThreads) void serve_tower_kernel(TowerArgs P) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const buf0 = smem;
    float* const buf1 = smem + kRows * P.stride0;
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4, l16 = lane & 15;
    const int b0 = blockIdx.x * kRows;
    const int nb = min(kRows, P.B - b0);

    // ---- the x tile -> buffer 0, rows past B and columns past K0 zero-filled up to the padded width ----
    {
        const int K0 = P.K0, Kp4 = pad_k(K0) / 4;
        for (int idx = (int)tid; idx < kRows * Kp4; idx += kThreads) {
            const int r = idx / Kp4, c = 4 * (idx - r * Kp4);
            float4 v = f4_zero();
            if (r < nb && c < K0) {
                const float* src = P.x + (size_t)(b0 + r) * K0 + c;
                if (P.vec_x) {
                    v = *reinterpret_cast<const float4*>(src);
                } else {
                    v.x = src[0];
                    if (c + 1 < K0) v.y = src[1];
                    if (c + 2 < K0) v.z = src[2];
                    if (c + 3 < K0) v.w = src[3];
                }
            }
            *reinterpret_cast<float4*>(buf0 + r * P.stride0 + c) = v;
        }
    }
    // ---- the first chunk of layer 0's weights ----
    float bq[kChunkRegs];
    {
        const int nt = tiles_of(P.units[0], wave);
#define SERVE_LOAD0(NT, CG) load_chunk<NT, CG>(bq, P.w[0], P.K0, P.units[0], 0, wave, l16, kq)
        SERVE_BY_TILES(nt, SERVE_LOAD0)
#undef SERVE_LOAD0
    }
    __syncthreads();

    int K = P.K0;
#pragma unroll 1
    for (int l = 0; l < P.L; ++l) {
        const int N = P.units[l];
        const int nt = tiles_of(N, wave);
        const float* A = (l & 1) ? buf1 : buf0;
        const int sa = (l & 1) ? P.stride1 : P.stride0;
        const bool last = l + 1 == P.L;
        // (the epilogue's per-column constants: requested ahead of the main loop)
        float sc[kMaxTiles], sh[kMaxTiles];
        const bool scaled = P.scale[l] != nullptr;
#pragma unroll
        for (int t = 0; t < kMaxTiles; ++t) {
            const int col = (int)(wave + kWaves * t) * 16 + (int)l16;
            sc[t] = (scaled && t < nt) ? P.scale[l][col] : 1.f;
            sh[t] = (scaled && t < nt) ? P.shift[l][col] : 0.f;
        }
        f32x4 acc[kMaxTiles];
#define SERVE_RUN(NT, CG) run_layer<NT, CG>(A, sa, P.w[l], P.b[l], K, N, bq, acc, wave, l16, kq)
        SERVE_BY_TILES(nt, SERVE_RUN)
#undef SERVE_RUN
        // ---- the next layer's first weights: in flight across the epilogue and the barrier ----
        if (!last) {
            const int nt2 = tiles_of(P.units[l + 1], wave);
#define SERVE_LOADN(NT, CG) load_chunk<NT, CG>(bq, P.w[l + 1], N, P.units[l + 1], 0, wave, l16, kq)
            SERVE_BY_TILES(nt2, SERVE_LOADN)
#undef SERVE_LOADN
        }
        // ---- epilogue: accumulator register r of lane (l16, kq) is row 4 kq + r of column tile * 16 + l16 ----
        const bool relu = (P.relu_bits >> l) & 1u;
        float* Hn = (l & 1) ? buf0 : buf1;
        const int sn = (l & 1) ? P.stride0 : P.stride1;
#pragma unroll
        for (int t = 0; t < kMaxTiles; ++t) {
            if (t < nt) {
                const int col = (int)(wave + kWaves * t) * 16 + (int)l16;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 4 * (int)kq + r;
                    float v = acc[t][r];
                    if (relu) v = fmaxf(v, 0.f);
                    if (scaled) v = fmaf(v, sc[t], sh[t]);
                    if (last) {
                        if (row < nb) P.out[(size_t)(b0 + row) * N + col] = v;
                    } else {
                        Hn[row * sn + col] = v;
                    }
                }
            }
        }
        if (!last) {
            // columns [N, pad_k(N)) of the next layer's input: exact zeros (its last chunk reads them)
            const int padw = pad_k(N) - N;
            for (int idx = (int)tid; idx < kRows * padw; idx += kThreads) {
                const int r = idx / padw;
                Hn[r * sn + N + (idx - r * padw)] = 0.f;
            }
            __syncthreads();
        }
        K = N;
    }
}

}  // namespace

RECALGO_EXPORT int recalgo_serve_abi_version(void) { return RECALGO_SERVE_ABI_VERSION; }

RECALGO_EXPORT int recalgo_serve_tower_supported(int K0, const int* units, int L) {
    if (!units || L < 1 || L > RECALGO_SERVE_MAX_LAYERS || K0 < 1 || K0 > RECALGO_SERVE_MAX_IN) return 0;
    for (int l = 0; l < L; ++l)
        if (units[l] < 16 || units[l] > RECALGO_SERVE_MAX_UNITS || units[l] % 16 != 0) return 0;
    return 1;
}

RECALGO_EXPORT int recalgo_serve_tower_fwd(const float* x, const float* const* w, const float* const* b, const float* const* scale,
                                           const float* const* shift, const int* units, int L, unsigned relu_bits, int B, int K0,
                                           float* out, recalgo_stream_t stream) {
    RECALGO_REQUIRE(recalgo_serve_tower_supported(K0, units, L) && B >= 1);
    RECALGO_REQUIRE(x && out && w);
    RECALGO_REQUIRE(aligned_to<4>(x, out));
    TowerArgs P = {};
    for (int l = 0; l < L; ++l) {
        P.w[l] = w[l];
        P.b[l] = b ? b[l] : nullptr;
        P.scale[l] = scale ? scale[l] : nullptr;
        P.shift[l] = (P.scale[l] && shift) ? shift[l] : nullptr;
        P.units[l] = units[l];
        RECALGO_REQUIRE(P.w[l] && (!P.scale[l] || P.shift[l]));
        RECALGO_REQUIRE(aligned_to<4>(P.w[l], P.b[l], P.scale[l], P.shift[l]));
    }
    P.x = x;
    P.out = out;
    P.L = L;
    P.relu_bits = relu_bits;
    P.B = B;
    P.K0 = K0;
    // layer l reads buffer l % 2 (K_l columns) and, unless it is the last, writes buffer (l + 1) % 2 (units[l] columns)
    int cols[2] = {pad_k(K0), 0};
    for (int l = 0; l + 1 < L; ++l) cols[(l + 1) & 1] = max(cols[(l + 1) & 1], pad_k(units[l]));
    P.stride0 = cols[0] + 4;
    P.stride1 = cols[1] ? cols[1] + 4 : 0;
    P.vec_x = (K0 % 4 == 0 && aligned16(x)) ? 1 : 0;
    const size_t lds = (size_t)kRows * (size_t)(P.stride0 + P.stride1) * sizeof(float);
    RECALGO_CHECK(launch_lds<serve_tower_kernel>(dim3(cdiv(B, kRows)), dim3(kThreads), lds, as_stream(stream), P));
    RECALGO_RETURN_LAST();
}
