// Loss tail (a14), TF1 Adam (a15), DIN activations (a12) — small streaming kernels, gfx950.
#include <algorithm>
#include <utility>
#include <vector>

#include "deferred.h"
#include "act.h"
#include "plan_scan.h"
#include "slab_sum.h"
#include "copy_span.h"
#include "../../include/recalgo_sumstep.h"
#include "sigmoid_ce.h"

namespace {

// ---------------------------------------------------------------------------------------
// sigmoid + mean sigmoid-CE + dlogit.  B is a few thousand: a single 1024-thread workgroup
// keeps the mean a deterministic tree reduction and needs no zero-initialised accumulator.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void sigmoid_ce_kernel(
    const float* __restrict__ logits, const float* __restrict__ labels, unsigned B,
    float grad_scale, float* __restrict__ prob, float* __restrict__ loss,
    float* __restrict__ dlogit) {
    __shared__ float red[16];
    // (the loop and the reduction tree: sigmoid_ce.h, shared with the multi-task tail of csrc/mmoe.hip)
    const float l = sigmoid_ce_task(
        logits, labels, B, grad_scale, dlogit != nullptr, red, [&](unsigned i, float p) { prob[i] = p; },
        [&](unsigned i, float d) { dlogit[i] = d; });
    if (threadIdx.x == 0) loss[0] = l;
}

// ---------------------------------------------------------------------------------------
// TF1 Adam, dense.  Pure stream: 4 reads + 3 writes (+ sparse zeroing of g) per element.
// ---------------------------------------------------------------------------------------
// (the update itself: deferred.h adam1 — shared with the sparse optimizer so that the deferred form stays bit-identical)
using recalgo_deferred::adam1;

__global__ __launch_bounds__(256) void adam_tf1_kernel(float* __restrict__ p, float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v,
                                                       int64_t n4, int64_t n, float lr_t_val,
                                                       const float* __restrict__ lr_t_dev, float b1,
                                                       float b2, float eps, int zero_grad) {
    const float lr_t = lr_t_dev ? lr_t_dev[0] : lr_t_val;
    const int64_t stride = (int64_t)gridDim.x * 256;
    float4* p4 = reinterpret_cast<float4*>(p);
    float4* g4 = reinterpret_cast<float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        float4 gg = g4[i];
        float4 mm = m4[i], vv = v4[i];
        // Exact shortcut of the dense update: where g, m and v are all zero (embedding rows no batch
        // has touched yet), m' = v' = 0 and p' = p - lr_t*0/(0+eps) = p — nothing to read or write.
        // TF1's dense semantics are kept bit for bit; only the traffic of inert words is skipped
        // (12 instead of 28 bytes per parameter).
        const bool inert = gg.x == 0.f && gg.y == 0.f && gg.z == 0.f && gg.w == 0.f && mm.x == 0.f && mm.y == 0.f &&
                           mm.z == 0.f && mm.w == 0.f && vv.x == 0.f && vv.y == 0.f && vv.z == 0.f && vv.w == 0.f;
        if (inert) continue;
        float4 pp = p4[i];
        adam1(pp.x, gg.x, mm.x, vv.x, lr_t, b1, b2, eps);
        adam1(pp.y, gg.y, mm.y, vv.y, lr_t, b1, b2, eps);
        adam1(pp.z, gg.z, mm.z, vv.z, lr_t, b1, b2, eps);
        adam1(pp.w, gg.w, mm.w, vv.w, lr_t, b1, b2, eps);
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
        if (zero_grad && (gg.x != 0.f || gg.y != 0.f || gg.z != 0.f || gg.w != 0.f)) g4[i] = f4_zero();
    }
    // tail (n % 4)
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)(n - n4 * 4)) {
        int64_t i = n4 * 4 + threadIdx.x;
        float pp = p[i], gg = g[i], mm = m[i], vv = v[i];
        adam1(pp, gg, mm, vv, lr_t, b1, b2, eps);
        p[i] = pp; m[i] = mm; v[i] = vv;
        if (zero_grad) g[i] = 0.f;
    }
}

// TF1 dense Adam over an embedding arena [rows, K] with a per-row liveness byte.  A row is inert
// until some batch first touches it (g != 0): until then g = m = v = 0 and the dense update is the
// identity, so nothing but g (to detect the first touch) and the byte is read.  Bit-identical to
// adam_tf1_kernel over the same buffers; invariant: live[r] == 0  =>  m[r,:] == v[r,:] == 0.
// K4 = K/4 lanes own one row (K4 divides 64, so a row never straddles a wave).
template <int K4>
__global__ __launch_bounds__(256) void adam_tf1_rows_kernel(float* __restrict__ p, float* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v,
                                                            unsigned char* __restrict__ live, int64_t total4,
                                                            float lr_t_val, const float* __restrict__ lr_t_dev,
                                                            float b1, float b2, float eps, int zero_grad) {
    const float lr_t = lr_t_dev ? lr_t_dev[0] : lr_t_val;
    const int64_t stride = (int64_t)gridDim.x * 256;
    float4* p4 = reinterpret_cast<float4*>(p);
    float4* g4 = reinterpret_cast<float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += stride) {
        const int64_t row = i / K4;
        float4 gg = g4[i];
        int nz = (gg.x != 0.f) | (gg.y != 0.f) | (gg.z != 0.f) | (gg.w != 0.f);
        int any = nz;
#pragma unroll
        for (int o = 1; o < K4; o <<= 1) any |= __shfl_xor(any, o, 64);
        const unsigned char was = live[row];
        if (!was && !any) continue;                       // inert row: identity update
        if (!was && (i % K4) == 0) live[row] = 1;
        float4 mm = m4[i], vv = v4[i], pp = p4[i];
        adam1(pp.x, gg.x, mm.x, vv.x, lr_t, b1, b2, eps);
        adam1(pp.y, gg.y, mm.y, vv.y, lr_t, b1, b2, eps);
        adam1(pp.z, gg.z, mm.z, vv.z, lr_t, b1, b2, eps);
        adam1(pp.w, gg.w, mm.w, vv.w, lr_t, b1, b2, eps);
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
        if (zero_grad && nz) g4[i] = f4_zero();
    }
}

// ---------------------------------------------------------------------------------------
// Live-row bookkeeping for embedding arenas (optimizer cost proportional to the
// rows a model has touched, with TF1's dense semantics kept exactly).
//   live[r] (one byte per row) == 1 and r is in list[0 .. count)  <=>  some gradient has reached row r.
// mark: every valid (b, f) id of a batch is checked; the first toucher of a row (atomicOr on the
// aligned 32-bit word holding the byte) appends it to the list.  adam_list: the dense TF1 update
// applied to the listed rows only — all other rows have g = m = v = 0, for which it is the identity.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mark_live_rows_kernel(const int64_t* __restrict__ ids,
                                                             const int64_t* __restrict__ row_base, int64_t n,
                                                             unsigned F, unsigned* __restrict__ live_words,
                                                             int* __restrict__ list, int* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t id = ids[i];
    if (id < 0) return;
    const int64_t row = id + (row_base ? row_base[i % F] : 0);
    const unsigned bit = 1u << (8 * (unsigned)(row & 3));
    unsigned* w = live_words + (row >> 2);
    if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) return;      // common case: already live
    const unsigned old = atomicOr(w, bit);
    if (!(old & bit)) list[atomicAdd(count, 1)] = (int)row;
}

// Address-ordered rebuild of the live-row list from the liveness bytes (housekeeping between steps:
// mark_live_rows appends in first-touch order, i.e. at random, and the list Adam then walks HBM at
// random — measured 40 us vs 32 us in address order for 345 k rows x 64 B x 7 streams).  Ordered
// compaction in three small launches: per-chunk popcounts, one-block exclusive scan of the chunk
// counts, ordered write.  A chunk = 1024 liveness words = 4096 rows, one word per thread and round.
constexpr unsigned kChunkWords = 1024;

__device__ __forceinline__ unsigned live_bytes_in(unsigned w) {       // number of non-zero bytes in a word
    return ((w & 0xffu) != 0) + ((w & 0xff00u) != 0) + ((w & 0xff0000u) != 0) + ((w & 0xff000000u) != 0);
}

__global__ __launch_bounds__(256) void live_chunk_count_kernel(const unsigned* __restrict__ live_words,
                                                               int64_t n_words, int* __restrict__ chunk_count) {
    __shared__ int part[4];
    const int64_t base = (int64_t)blockIdx.x * kChunkWords;
    int c = 0;
#pragma unroll
    for (unsigned r = 0; r < kChunkWords / 256; ++r) {
        const int64_t w = base + r * 256 + threadIdx.x;
        if (w < n_words) c += (int)live_bytes_in(live_words[w]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// exclusive scan of chunk_count in place, total -> live_count[0]; one block, any number of chunks
__global__ __launch_bounds__(1024) void live_chunk_scan_kernel(int* __restrict__ chunk_count, int n_chunks,
                                                               int* __restrict__ live_count) {
    __shared__ int wave_tot[16];
    __shared__ int carry_s;
    const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < n_chunks; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const int x = i < n_chunks ? chunk_count[i] : 0;
        int incl = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o, 64);
            if ((int)lane >= o) incl += y;
        }
        if (lane == 63) wave_tot[wv] = incl;
        __syncthreads();
        int before = carry_s;
        for (unsigned k = 0; k < wv; ++k) before += wave_tot[k];
        if (i < n_chunks) chunk_count[i] = before + incl - x;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) live_count[0] = carry_s;
}

__global__ __launch_bounds__(256) void live_chunk_write_kernel(const unsigned* __restrict__ live_words,
                                                               int64_t n_words, int64_t rows,
                                                               const int* __restrict__ chunk_base,
                                                               int* __restrict__ list) {
    __shared__ int wave_tot[4];
    const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * kChunkWords;
    int out = chunk_base[blockIdx.x];
    for (unsigned r = 0; r < kChunkWords / 256; ++r) {
        const int64_t w = base + r * 256 + threadIdx.x;
        const unsigned word = w < n_words ? live_words[w] : 0u;
        const int x = (int)live_bytes_in(word);
        int incl = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o, 64);
            if ((int)lane >= o) incl += y;
        }
        if (lane == 63) wave_tot[wv] = incl;
        __syncthreads();
        int pos = out + incl - x;
        for (unsigned k = 0; k < wv; ++k) pos += wave_tot[k];
#pragma unroll
        for (unsigned b = 0; b < 4; ++b)
            if ((word >> (8 * b)) & 0xffu) {
                const int64_t row = w * 4 + b;
                if (row < rows) list[pos++] = (int)row;
            }
        out += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
        __syncthreads();
    }
}

template <int K4>
__global__ __launch_bounds__(256) void adam_tf1_list_kernel(float* __restrict__ p, float* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v,
                                                            const int* __restrict__ list,
                                                            const int* __restrict__ count, float lr_t_val,
                                                            const float* __restrict__ lr_t_dev, float b1,
                                                            float b2, float eps, int zero_grad) {
    const float lr_t = lr_t_dev ? lr_t_dev[0] : lr_t_val;
    const int64_t total4 = (int64_t)count[0] * K4;
    const int64_t stride = (int64_t)gridDim.x * 256;
    float4* p4 = reinterpret_cast<float4*>(p);
    float4* g4 = reinterpret_cast<float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total4; t += stride) {
        const int64_t i = (int64_t)list[t / K4] * K4 + (t % K4);
        float4 gg = g4[i], mm = m4[i], vv = v4[i], pp = p4[i];
        const bool nz = gg.x != 0.f || gg.y != 0.f || gg.z != 0.f || gg.w != 0.f;
        adam1(pp.x, gg.x, mm.x, vv.x, lr_t, b1, b2, eps);
        adam1(pp.y, gg.y, mm.y, vv.y, lr_t, b1, b2, eps);
        adam1(pp.z, gg.z, mm.z, vv.z, lr_t, b1, b2, eps);
        adam1(pp.w, gg.w, mm.w, vv.w, lr_t, b1, b2, eps);
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
        if (zero_grad && nz) g4[i] = f4_zero();
    }
}

// ---------------------------------------------------------------------------------------
// PReLU / Dice (algorithm/DIN/activations.py:4-37), x: [rows, C], alpha: [C].
// ---------------------------------------------------------------------------------------
using recalgo_act::kDiceInvStd;                      // 1/sqrt(1 + 1e-3): BN inference, stats (0,1)

template <bool DICE>
__global__ __launch_bounds__(256) void act_fwd_kernel(const float* __restrict__ x,
                                                      const float* __restrict__ alpha, int64_t n,
                                                      unsigned C, float* __restrict__ y) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float xv = x[i], a = alpha[i % C];
    if (DICE) {
        float px = 1.0f / (1.0f + expf(-xv * kDiceInvStd));
        y[i] = xv * px + a * xv * (1.0f - px);
    } else {
        y[i] = fmaxf(0.f, xv) + a * fminf(0.f, xv);
    }
}

// dx and per-workgroup partial dalpha ([gridDim.x][C], rows of one workgroup are contiguous).
template <bool DICE>
__global__ __launch_bounds__(256) void act_bwd_kernel(const float* __restrict__ x,
                                                      const float* __restrict__ alpha,
                                                      const float* __restrict__ gy, unsigned rows,
                                                      unsigned C, unsigned rows_per_blk,
                                                      float* __restrict__ dx,
                                                      float* __restrict__ partial) {
    const unsigned r0 = blockIdx.x * rows_per_blk;
    const unsigned r1 = min(rows, r0 + rows_per_blk);
    for (unsigned c = threadIdx.x; c < C; c += 256) {
        float a = alpha[c], da = 0.f;
        for (unsigned r = r0; r < r1; ++r) {
            size_t i = (size_t)r * C + c;
            float xv = x[i], g = gy[i];
            if (DICE) {
                float px = 1.0f / (1.0f + expf(-xv * kDiceInvStd));
                float dpx = px * (1.0f - px) * kDiceInvStd;
                // y = x*px + a*x*(1-px)
                dx[i] = g * (px + a * (1.0f - px) + xv * dpx * (1.0f - a));
                da += g * xv * (1.0f - px);
            } else {
                dx[i] = g * (xv > 0.f ? 1.0f : (xv < 0.f ? a : 0.f));
                da += g * fminf(0.f, xv);
            }
        }
        partial[(size_t)blockIdx.x * C + c] = da;
    }
}

constexpr unsigned kActRowsPerBlk = 16;

// C % 4 == 0: the same pass on 64-row x 64-column tiles (16 float4 column groups x 16 row lanes, 4
// rows per thread): 8x the workgroups of the row-block kernel for a [4096, 128] layer and 4x fewer
// partial rows for the fixed-order dalpha sum.
constexpr unsigned kActTileRows = 64;
template <bool DICE>
__global__ __launch_bounds__(256) void act_bwd_tile_kernel(const float4* __restrict__ x,
                                                           const float4* __restrict__ alpha,
                                                           const float4* __restrict__ gy, unsigned rows,
                                                           unsigned C4, float4* __restrict__ dx,
                                                           float4* __restrict__ partial) {
    __shared__ float4 sh[256];
    const unsigned cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const unsigned c4 = blockIdx.x * 16 + cl;
    const unsigned r0 = blockIdx.y * kActTileRows;
    float4 da = f4_zero();
    if (c4 < C4) {
        const float4 a4 = alpha[c4];
        const float a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (unsigned k = 0; k < kActTileRows / 16; ++k) {
            const unsigned r = r0 + rl + 16 * k;
            if (r < rows) {
                const size_t i = (size_t)r * C4 + c4;
                const float4 x4 = x[i], g4 = gy[i];
                const float xv[4] = {x4.x, x4.y, x4.z, x4.w}, g[4] = {g4.x, g4.y, g4.z, g4.w};
                float o[4], d[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (DICE) {
                        const float px = 1.0f / (1.0f + expf(-xv[j] * kDiceInvStd));
                        const float dpx = px * (1.0f - px) * kDiceInvStd;
                        o[j] = g[j] * (px + a[j] * (1.0f - px) + xv[j] * dpx * (1.0f - a[j]));
                        d[j] = g[j] * xv[j] * (1.0f - px);
                    } else {
                        o[j] = g[j] * (xv[j] > 0.f ? 1.0f : (xv[j] < 0.f ? a[j] : 0.f));
                        d[j] = g[j] * fminf(0.f, xv[j]);
                    }
                }
                dx[i] = make_float4(o[0], o[1], o[2], o[3]);
                da = f4_add(da, make_float4(d[0], d[1], d[2], d[3]));
            }
        }
    }
    sh[threadIdx.x] = da;
    __syncthreads();
    if (rl == 0 && c4 < C4) {
        float4 t = sh[cl];
#pragma unroll
        for (unsigned k = 1; k < 16; ++k) t = f4_add(t, sh[k * 16 + cl]);
        partial[(size_t)blockIdx.y * C4 + c4] = t;
    }
}

// ---------------------------------------------------------------------------------------
// One launch per optimizer step: the step counter, TF1 Adam over the flat dense-variable buffer and
// over the live rows of up to kAdamMaxArenas embedding arenas (previously adam_advance + adam_tf1 +
// one adam_tf1_list per arena: 3-4 launches of 5-30 us, the first two at the launch floor).
// Every workgroup reads step[0] when it starts and derives lr_t itself (two pow and a sqrt in double);
// the LAST workgroup to finish (arrival ticket) publishes step[0] = t and re-arms the ticket — by then
// every workgroup has read the old value, so there is no race, and the next launch (a kernel boundary
// later) sees the new one.  hipGraph replayable: nothing depends on host-side state.
// ---------------------------------------------------------------------------------------
constexpr int kAdamMaxArenas = 4;
struct AdamArena {
    float* p; float* g; float* m; float* v;
    const int* list;
    const int* count;
    int K;
    int k4_shift;             // log2(K / 4) when K / 4 is a power of two, else -1
    int lazy;                 // LazyAdam: rows whose gradient is all zero this step are left untouched
    unsigned first_block, n_blocks;
};
struct AdamStepArgs {
    float* p; float* g; float* m; float* v;        // flat dense buffer (n may be 0)
    long long n;
    unsigned dense_blocks;
    AdamArena ar[kAdamMaxArenas];
    int n_arenas;
    long long* step;
    int* ticket;
    int advance;
    float lr, b1, b2, eps;
    int zero_grad;
    // the scatter plans of the arenas on the owner-computes path (sparse.hip): one extra workgroup each turns the plan's bucket
    // totals into the prefix `place` needs — this launch runs between the step's last count and `place` anyway
    recalgo_plan::Scan scan[kAdamMaxArenas];
    unsigned scan_first;      // blocks [scan_first, scan_first + n_scans) are those workgroups
};

// float4 words [lo4, hi4) of the flat dense buffer, by workgroup `blk` of `nblk`
__device__ __forceinline__ void adam_dense_words(const AdamStepArgs& A, long long lo4, long long hi4, unsigned blk, unsigned nblk,
                                                 float lr_t, float b1, float b2, float eps) {
    const long long stride = (long long)nblk * 256;
    float4* p4 = reinterpret_cast<float4*>(A.p);
    float4* g4 = reinterpret_cast<float4*>(A.g);
    float4* m4 = reinterpret_cast<float4*>(A.m);
    float4* v4 = reinterpret_cast<float4*>(A.v);
    for (long long i = lo4 + (long long)blk * 256 + threadIdx.x; i < hi4; i += stride) {
        float4 gg = g4[i], mm = m4[i], vv = v4[i];
        const bool inert = gg.x == 0.f && gg.y == 0.f && gg.z == 0.f && gg.w == 0.f && mm.x == 0.f && mm.y == 0.f &&
                           mm.z == 0.f && mm.w == 0.f && vv.x == 0.f && vv.y == 0.f && vv.z == 0.f && vv.w == 0.f;
        if (inert) continue;                       // exact: the update of an all-zero word is the identity
        float4 pp = p4[i];
        adam1(pp.x, gg.x, mm.x, vv.x, lr_t, b1, b2, eps);
        adam1(pp.y, gg.y, mm.y, vv.y, lr_t, b1, b2, eps);
        adam1(pp.z, gg.z, mm.z, vv.z, lr_t, b1, b2, eps);
        adam1(pp.w, gg.w, mm.w, vv.w, lr_t, b1, b2, eps);
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
        if (A.zero_grad && (gg.x != 0.f || gg.y != 0.f || gg.z != 0.f || gg.w != 0.f)) g4[i] = f4_zero();
    }
}
// one element outside the float4 words (the n % 4 tail)
__device__ __forceinline__ void adam_dense_element(const AdamStepArgs& A, long long i, float lr_t, float b1, float b2, float eps) {
    float pp = A.p[i], gg = A.g[i], mm = A.m[i], vv = A.v[i];
    adam1(pp, gg, mm, vv, lr_t, b1, b2, eps);
    A.p[i] = pp; A.m[i] = mm; A.v[i] = vv;
    if (A.zero_grad) A.g[i] = 0.f;
}

// the live rows of the arena that workgroup `bid` of the launch belongs to (A.n_arenas > 0, bid >= A.dense_blocks)
__device__ __forceinline__ void adam_arena_block(const AdamStepArgs& A, unsigned bid, float lr_t, float b1, float b2, float eps) {
    int a = 0;
#pragma unroll
    for (int k = 1; k < kAdamMaxArenas; ++k)
        if (k < A.n_arenas && bid >= A.ar[k].first_block) a = k;
    AdamArena R = A.ar[0];                       // select by value (a dynamic index into the kernel arguments
#pragma unroll                                       // would go through scratch)
    for (int k = 1; k < kAdamMaxArenas; ++k)
        if (a == k) R = A.ar[k];
    const unsigned blk = bid - R.first_block;
    const long long stride = (long long)R.n_blocks * 256;
    const int K = R.K;
    if ((K & 3) == 0) {
        const int K4 = K >> 2;
        const long long total4 = (long long)R.count[0] * K4;
        float4* p4 = reinterpret_cast<float4*>(R.p);
        float4* g4 = reinterpret_cast<float4*>(R.g);
        float4* m4 = reinterpret_cast<float4*>(R.m);
        float4* v4 = reinterpret_cast<float4*>(R.v);
        const int sh = R.k4_shift;
        for (long long tt = (long long)blk * 256 + threadIdx.x; tt < total4; tt += stride) {
            const long long r = sh >= 0 ? tt >> sh : tt / K4;
            const long long i = (long long)R.list[r] * K4 + (tt - r * K4);
            float4 gg = g4[i];
            const bool nz = gg.x != 0.f || gg.y != 0.f || gg.z != 0.f || gg.w != 0.f;
            if (R.lazy) {
                // tf.contrib.opt.LazyAdamOptimizer (the reference's DIEN, dien.py:328): only the rows of this step's
                // IndexedSlices move — here: rows with a non-zero gradient (the K4 lanes of a row vote)
                int any = nz;
                if (sh > 0)
                    for (int o = 1; o < K4; o <<= 1) any |= __shfl_xor(any, o, 64);
                if (!any) continue;
            }
            float4 mm = m4[i], vv = v4[i], pp = p4[i];
            adam1(pp.x, gg.x, mm.x, vv.x, lr_t, b1, b2, eps);
            adam1(pp.y, gg.y, mm.y, vv.y, lr_t, b1, b2, eps);
            adam1(pp.z, gg.z, mm.z, vv.z, lr_t, b1, b2, eps);
            adam1(pp.w, gg.w, mm.w, vv.w, lr_t, b1, b2, eps);
            p4[i] = pp; m4[i] = mm; v4[i] = vv;
            if (A.zero_grad && nz) g4[i] = f4_zero();
        }
    } else {
        const long long total = (long long)R.count[0] * K;
        for (long long tt = (long long)blk * 256 + threadIdx.x; tt < total; tt += stride) {
            const long long r = tt / K;
            const long long i = (long long)R.list[r] * K + (tt - r * K);
            float gg = R.g[i];
            const bool nz = gg != 0.f;
            if (R.lazy && !nz) continue;                 // (element-wise vote for widths that are not 4 * 2^n)
            float mm = R.m[i], vv = R.v[i], pp = R.p[i];
            adam1(pp, gg, mm, vv, lr_t, b1, b2, eps);
            R.p[i] = pp; R.m[i] = mm; R.v[i] = vv;
            if (A.zero_grad && nz) R.g[i] = 0.f;
        }
    }
}

// the last workgroup to arrive publishes the new step count (every workgroup in front of scan_first, once, at its end)
__device__ __forceinline__ void adam_publish_step(const AdamStepArgs& A, long long t) {
    __syncthreads();
    if (threadIdx.x == 0) {
        const int arrived = __hip_atomic_fetch_add(A.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (arrived == (int)A.scan_first - 1) {                 // (the plan-scan workgroups behind scan_first take no ticket)
            __hip_atomic_store(A.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            A.step[0] = t;
        }
    }
}

__device__ __forceinline__ float adam_lr_t_value(const AdamStepArgs& A, long long t) {
    const double td = (double)t;
    return (float)((double)A.lr * sqrt(1.0 - pow((double)A.b2, td)) / (1.0 - pow((double)A.b1, td)));
}
// lr_t of step t, derived by every workgroup itself (two pow and a sqrt in double); s_lr_t: one float of LDS
__device__ __forceinline__ float adam_lr_t(const AdamStepArgs& A, long long t, float* s_lr_t) {
    if (threadIdx.x == 0) *s_lr_t = adam_lr_t_value(A, t);
    __syncthreads();
    return *s_lr_t;
}

__global__ __launch_bounds__(256) void adam_tf1_step_kernel(AdamStepArgs A) {
    __shared__ float s_lr_t;
    if (blockIdx.x >= A.scan_first) {                          // (workgroup-uniform)
        __shared__ unsigned scan_sh[8];
        recalgo_plan::scan_block(A.scan[blockIdx.x - A.scan_first], scan_sh);
        return;
    }
    const long long t = A.step[0] + (A.advance ? 1 : 0);
    const float lr_t = adam_lr_t(A, t, &s_lr_t), b1 = A.b1, b2 = A.b2, eps = A.eps;
    if (blockIdx.x < A.dense_blocks) {
        const long long n4 = A.n / 4;
        adam_dense_words(A, 0, n4, blockIdx.x, A.dense_blocks, lr_t, b1, b2, eps);
        if (blockIdx.x == 0 && threadIdx.x < (unsigned)(A.n - n4 * 4)) adam_dense_element(A, n4 * 4 + threadIdx.x, lr_t, b1, b2, eps);
    } else if (A.n_arenas > 0) {                     // (n == 0 and no arena: the one workgroup only takes its ticket —
        adam_arena_block(A, blockIdx.x, lr_t, b1, b2, eps);      //  ar[0] is then a padding descriptor with no count to read)
    }
    if (A.advance) adam_publish_step(A, t);
}

// ---------------------------------------------------------------------------------------
// The step's deferred sums AND the optimizer launch above in one: a weight gradient that the backward pass left as split slabs or
// partial rows is summed (slab_sum.h: the order of dense_sum_slabs_kernel) by the thread that then updates the parameter — the sum
// launch wrote it to the flat gradient buffer only for this launch to read it back once, a kernel boundary later.
// Workgroups: [the jobs' (first_block, the layout of the sum launch) | "rest": the intervals of the flat buffer no job writes,
// their gradient read from the buffer as above | arenas | plan scans].  A job whose output lies outside the flat buffer (the loss
// value) is only summed.  p, m, v of a job's element are requested before its slabs, so that all the loads are in flight together.
// ---------------------------------------------------------------------------------------
constexpr int kSumStepMaxJobs = recalgo_slabs::kMaxSplitJobs;
constexpr int kSumStepMaxRest = 2 * kSumStepMaxJobs + 1;     // (the complement of <= 2 outputs per job)
struct SumStepArgs {
    AdamStepArgs A;                // A.dense_blocks = job_blocks + rest_blocks
    recalgo_slabs::SplitJob job[kSumStepMaxJobs];
    int n_jobs, n_rest;
    unsigned job_blocks, rest_blocks;
    unsigned lr_block;             // the workgroup behind the plan scans that leaves the next step's lr_t (no ticket buffer: none)
    long long rest_lo[kSumStepMaxRest], rest_hi[kSumStepMaxRest];     // element intervals [lo, hi) of the flat buffer
};
static_assert(sizeof(SumStepArgs) <= 4096, "passed by value: the kernel-argument segment");

// what the optimizer launch does with one summed element e of the flat buffer / one float4 word e4 (p, m, v loaded by the caller)
__device__ __forceinline__ void sum_step_finish1(const AdamStepArgs& A, size_t e, float gg, float pp, float mm, float vv, float lr_t) {
    if (!(gg == 0.f && mm == 0.f && vv == 0.f)) {
        adam1(pp, gg, mm, vv, lr_t, A.b1, A.b2, A.eps);
        A.p[e] = pp; A.m[e] = mm; A.v[e] = vv;
    }
    A.g[e] = (A.zero_grad && gg != 0.f) ? 0.f : gg;
}
__device__ __forceinline__ void sum_step_finish4(const AdamStepArgs& A, size_t e4, float4 gg, float4 pp, float4 mm, float4 vv, float lr_t) {
    const float b1 = A.b1, b2 = A.b2, eps = A.eps;
    const bool nz = gg.x != 0.f || gg.y != 0.f || gg.z != 0.f || gg.w != 0.f;
    const bool inert = !nz && mm.x == 0.f && mm.y == 0.f && mm.z == 0.f && mm.w == 0.f && vv.x == 0.f && vv.y == 0.f &&
                       vv.z == 0.f && vv.w == 0.f;
    if (!inert) {
        adam1(pp.x, gg.x, mm.x, vv.x, lr_t, b1, b2, eps);
        adam1(pp.y, gg.y, mm.y, vv.y, lr_t, b1, b2, eps);
        adam1(pp.z, gg.z, mm.z, vv.z, lr_t, b1, b2, eps);
        adam1(pp.w, gg.w, mm.w, vv.w, lr_t, b1, b2, eps);
        reinterpret_cast<float4*>(A.p)[e4] = pp;
        reinterpret_cast<float4*>(A.m)[e4] = mm;
        reinterpret_cast<float4*>(A.v)[e4] = vv;
    }
    reinterpret_cast<float4*>(A.g)[e4] = (A.zero_grad && nz) ? f4_zero() : gg;   // (what sum + step leave: the sum, or zero_grad's zeros)
}

// The arrival ticket of this launch, sharded: its several hundred workgroups end within a microsecond of each other, and one
// word takes an atomic every ~12 ns (all of them on one ticket made the launch 15.3 us, the sum of the two it replaces 14.2).
// A workgroup arrives at shard blockIdx % 8 (a word on a line of its own); the last of a shard re-arms it and arrives at the top
// word, the last there re-arms that and publishes the step count.
constexpr int kTicketShards = 8;
constexpr int kTicketStride = 64;                                    // ints between two words: 256 bytes
constexpr int kTicketInts = kTicketStride * (kTicketShards + 3);      // (recalgo_adam_tf1_sum_step_workspace_bytes)
// Behind the ticket words, two slots {t, lr, b1, b2 -> lr_t}: lr_t costs two pow and a sqrt in double behind the load of the
// counter (~2.5 us in front of a workgroup's first slab load).  One extra workgroup of the launch of step t leaves lr_t of step
// t + 1 in slot (t + 1) & 1 (nobody reads that slot in this launch); the workgroups of the next launch find it there, compare the
// whole key, and compute lr_t themselves where it does not match (the first step, a counter set from outside).
struct LrSlot { int t_lo, t_hi, lr, b1, b2, lr_t; };
__device__ __forceinline__ int* lr_slot(const AdamStepArgs& A, int k) { return A.ticket + (kTicketShards + 1 + k) * kTicketStride; }
__device__ __forceinline__ void sum_step_publish(const AdamStepArgs& A, long long t) {
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned total = A.scan_first, s = blockIdx.x % kTicketShards;         // (the scan workgroups take no ticket)
        const unsigned in_shard = (total - s + kTicketShards - 1) / kTicketShards;   // workgroups b < total with b % 8 == s
        int* shard = A.ticket + (1 + s) * kTicketStride;
        if (__hip_atomic_fetch_add(shard, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)in_shard - 1) {
            __hip_atomic_store(shard, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned shards = total < (unsigned)kTicketShards ? total : (unsigned)kTicketShards;
            if (__hip_atomic_fetch_add(A.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)shards - 1) {
                __hip_atomic_store(A.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                A.step[0] = t;
            }
        }
    }
}

// (the name ends in adam_tf1_step_kernel: bench.in_step_table counts a profile's steps by the launches of that name)
__global__ __launch_bounds__(256) void sums_adam_tf1_step_kernel(SumStepArgs K) {
    const AdamStepArgs& A = K.A;
    __shared__ float s_lr_t;
    if (blockIdx.x >= A.scan_first && blockIdx.x != K.lr_block) {     // (workgroup-uniform, as every branch on blockIdx below)
        __shared__ unsigned scan_sh[8];
        recalgo_plan::scan_block(A.scan[blockIdx.x - A.scan_first], scan_sh);
        return;
    }
    if (blockIdx.x == K.lr_block) {                            // lr_t of the NEXT step (see LrSlot)
        if (threadIdx.x == 0) {
            const long long tn = A.step[0] + (A.advance ? 2 : 1);
            int* o = lr_slot(A, (int)(tn & 1));
            o[0] = (int)tn; o[1] = (int)(tn >> 32); o[2] = __float_as_int(A.lr); o[3] = __float_as_int(A.b1);
            o[4] = __float_as_int(A.b2); o[5] = __float_as_int(adam_lr_t_value(A, tn));
        }
        return;
    }
    // (both slots are requested with the counter: no load depends on another)
    LrSlot c0{}, c1{};
    if (A.ticket != nullptr) {
        const int* a = lr_slot(A, 0);
        const int* b = lr_slot(A, 1);
        c0 = LrSlot{a[0], a[1], a[2], a[3], a[4], a[5]};
        c1 = LrSlot{b[0], b[1], b[2], b[3], b[4], b[5]};
    }
    const long long t = A.step[0] + (A.advance ? 1 : 0);
    const LrSlot c = (t & 1) ? c1 : c0;
    const bool cached = A.ticket != nullptr && c.t_lo == (int)t && c.t_hi == (int)(t >> 32) && c.lr == __float_as_int(A.lr) &&
                        c.b1 == __float_as_int(A.b1) && c.b2 == __float_as_int(A.b2);           // (uniform over the whole grid)
    const float lr_t = cached ? __int_as_float(c.lr_t) : adam_lr_t(A, t, &s_lr_t);
    if (blockIdx.x < K.job_blocks) {
        int j = 0;
#pragma unroll
        for (int k = 1; k < kSumStepMaxJobs; ++k)
            if (k < K.n_jobs && blockIdx.x >= K.job[k].first_block) j = k;
        const recalgo_slabs::SplitJob& jb = K.job[j];
        const size_t blk = blockIdx.x - jb.first_block;
        const unsigned long long flat_bytes = (unsigned long long)A.n * sizeof(float);
        if (jb.vec == 2) {
            __shared__ float sh[16][17];
            const size_t c = blk * 16 + (threadIdx.x & 15);
            const bool writer = (threadIdx.x >> 4) == 0 && c < jb.n;
            // (byte offset into the flat gradient buffer; an output outside it wraps to a large number)
            const unsigned long long off = (unsigned long long)(reinterpret_cast<uintptr_t>(jb.out0 + c) - reinterpret_cast<uintptr_t>(A.g));
            const bool flat = writer && off < flat_bytes;
            const size_t e = (size_t)(off / sizeof(float));
            float pp = 0.f, mm = 0.f, vv = 0.f;
            if (flat) { pp = A.p[e]; mm = A.m[e]; vv = A.v[e]; }
            const float gg = recalgo_slabs::sum_tall(jb, blk, sh);
            if (flat) sum_step_finish1(A, e, gg, pp, mm, vv, lr_t);
            else if (writer) jb.out0[c] = gg;
        } else if (jb.vec) {
            const size_t i = (blk * 256 + threadIdx.x) * 4;
            if (i < jb.n) {
                const size_t e4 = (size_t)(recalgo_slabs::job_target(jb, i) - A.g) / 4;
                const float4 pp = reinterpret_cast<const float4*>(A.p)[e4], mm = reinterpret_cast<const float4*>(A.m)[e4],
                             vv = reinterpret_cast<const float4*>(A.v)[e4];
                sum_step_finish4(A, e4, recalgo_slabs::sum_slabs4(jb, i), pp, mm, vv, lr_t);
            }
        } else {
            const size_t i = blk * 256 + threadIdx.x;
            if (i < jb.n) {
                const size_t e = (size_t)(recalgo_slabs::job_target(jb, i) - A.g);
                const float pp = A.p[e], mm = A.m[e], vv = A.v[e];
                sum_step_finish1(A, e, recalgo_slabs::sum_slabs1(jb, i), pp, mm, vv, lr_t);
            }
        }
    } else if (blockIdx.x < A.dense_blocks) {
        const unsigned blk = blockIdx.x - K.job_blocks;
        for (int k = 0; k < K.n_rest; ++k) {
            const long long lo = K.rest_lo[k], hi = K.rest_hi[k];
            const long long lo4 = (lo + 3) >> 2, hi4 = hi >> 2;
            if (lo4 < hi4) adam_dense_words(A, lo4, hi4, blk, K.rest_blocks, lr_t, A.b1, A.b2, A.eps);
            if (blk == 0 && threadIdx.x < 8) {
                // the elements in front of the first whole word (threads 0-2) and behind the last (threads 4-6)
                const long long head_end = lo4 * 4 < hi ? lo4 * 4 : hi, tail_lo = hi4 * 4 > head_end ? hi4 * 4 : head_end;
                const long long i = threadIdx.x < 4 ? lo + threadIdx.x : tail_lo + (threadIdx.x - 4);
                if (i < (threadIdx.x < 4 ? head_end : hi)) adam_dense_element(A, i, lr_t, A.b1, A.b2, A.eps);
            }
        }
    } else if (A.n_arenas > 0) {
        adam_arena_block(A, blockIdx.x, lr_t, A.b1, A.b2, A.eps);
    }
    if (A.advance) sum_step_publish(A, t);
}

__global__ void adam_advance_kernel(int64_t* step, float lr, float b1, float b2, float* lr_t) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int64_t t = step[0] + 1;
        step[0] = t;
        double td = (double)t;
        lr_t[0] = (float)((double)lr * sqrt(1.0 - pow((double)b2, td)) / (1.0 - pow((double)b1, td)));
    }
}
// ---------------------------------------------------------------------------------------
// tf.concat of up to 4 row-major [B, w_p] parts + the value of DIN's mini-batch-aware regulariser over the result
// (din.py:249-257: l2_lambda / 2 / B * sum(ev^2), ev = concat[category, target, attention output]) in ONE launch:
// a workgroup copies a block of rows and accumulates their squares; per-workgroup partial sums are added IN FIXED ORDER by
// the workgroup that arrives last (ticket), so the scalar is bit-reproducible.  Replaces a concat copy, a dot product
// (two library launches) and a scaling launch.
// ---------------------------------------------------------------------------------------
constexpr int kCatMaxParts = 4;
struct CatArgs {
    const float* x[kCatMaxParts];
    int width[kCatMaxParts], off[kCatMaxParts];
    int n, B, C;              // C = total width (the row stride of `out`)
    float* out;
    float scale;
    float* sum_out;           // scale * sum(out^2)
    float* partials;          // [gridDim.x]
    unsigned* ticket;         // zero before the first launch; the last workgroup leaves it zero again
    int rows_per_block;
};
__global__ __launch_bounds__(256) void concat_sumsq_kernel(CatArgs A) {
    __shared__ float red[4];
    __shared__ unsigned s_last;
    const int r0 = blockIdx.x * A.rows_per_block, r1 = min(A.B, r0 + A.rows_per_block);
    float acc = 0.f;
    for (int p = 0; p < A.n; ++p) {
        const int w = A.width[p], n = (r1 - r0) * w;
        const float* __restrict__ src = A.x[p] + (size_t)r0 * w;
        float* __restrict__ dst = A.out + (size_t)r0 * A.C + A.off[p];
        if ((w & 3) == 0 && (A.C & 3) == 0 && (A.off[p] & 3) == 0 && (reinterpret_cast<uintptr_t>(A.x[p]) & 15) == 0 &&
            (reinterpret_cast<uintptr_t>(A.out) & 15) == 0) {
            const int w4 = w >> 2;
            for (int i = threadIdx.x; i < (n >> 2); i += 256) {
                const int r = i / w4, c = i - r * w4;
                const float4 v = reinterpret_cast<const float4*>(src)[i];
                *reinterpret_cast<float4*>(dst + (size_t)r * A.C + 4 * c) = v;
                acc = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, acc))));
            }
        } else {
            for (int i = threadIdx.x; i < n; i += 256) {
                const int r = i / w, c = i - r * w;
                const float v = src[i];
                dst[(size_t)r * A.C + c] = v;
                acc = fmaf(v, v, acc);
            }
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        // publish the partial with a write-through (sc1) store, drain it, then draw a ticket; the workgroup that draws the last
        // ticket reads every partial with sc1 loads (guides/cdna_hip_programming.md Guideline 16, the drained-sc1 form: no
        // release fence — a fence would first write back the 27 KB of `out` this workgroup has just dirtied, ~6 us)
        __hip_atomic_store(&A.partials[blockIdx.x], (red[0] + red[1]) + (red[2] + red[3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(A.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = t == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    // fixed order: thread t adds partials t, t + 256, ...; then the 256 thread sums in thread order
    float tot = 0.f;
    for (unsigned i = threadIdx.x; i < gridDim.x; i += 256)
        tot += __hip_atomic_load(&A.partials[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __shared__ float all[256];
    all[threadIdx.x] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t2 = 0.f;
        for (int i = 0; i < 256; ++i) t2 += all[i];
        A.sum_out[0] = A.scale * t2;
        __hip_atomic_store(A.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

RECALGO_EXPORT int64_t recalgo_concat_sumsq_workspace_bytes(int B) {
    // ticket word + padding to word 16, then one partial per workgroup (B == 0 still launches one workgroup)
    return (int64_t)((B > 0 ? cdiv(B, 16) : 1) + 16) * 4;
}
RECALGO_EXPORT int recalgo_concat_sumsq(const float* const* parts, const int* widths, int n_parts, int B, float* out,
                                        float scale, float* sum_out, void* workspace, recalgo_stream_t stream) {
    // (an empty batch has no rows to copy: its parts and `out` may be null; the sum is still written)
    RECALGO_REQUIRE(parts && widths && n_parts >= 1 && n_parts <= kCatMaxParts && B >= 0 && (out || B == 0) && sum_out && workspace);
    CatArgs A;
    int C = 0;
    for (int p = 0; p < kCatMaxParts; ++p) {
        A.x[p] = p < n_parts ? parts[p] : nullptr;
        A.width[p] = p < n_parts ? widths[p] : 0;
        A.off[p] = C;
        if (p < n_parts) {
            RECALGO_REQUIRE((parts[p] != nullptr || B == 0) && widths[p] >= 1);
            C += widths[p];
        }
    }
    A.n = n_parts; A.B = B; A.C = C; A.out = out; A.scale = scale; A.sum_out = sum_out;
    A.rows_per_block = 16;
    const int blocks = B > 0 ? cdiv(B, A.rows_per_block) : 1;
    A.ticket = static_cast<unsigned*>(workspace);             // word 0 (zero-initialised by the caller, once)
    A.partials = reinterpret_cast<float*>(static_cast<unsigned*>(workspace) + 16);
    hipLaunchKernelGGL(concat_sumsq_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), A);
    RECALGO_RETURN_LAST();
}

namespace {
}  // namespace

namespace {
// 16 bytes per thread and pass (8 in flight per thread for large spans); a head / tail of single bytes for any alignment
__global__ __launch_bounds__(256) void copy_bytes_kernel(unsigned char* __restrict__ dst, const unsigned char* __restrict__ src,
                                                         size_t head, size_t n16, size_t nbytes) {
    recalgo_copy::copy_span(dst, src, head, n16, nbytes, (size_t)blockIdx.x * 256 + threadIdx.x, (size_t)gridDim.x * 256);
}
}  // namespace

RECALGO_EXPORT int recalgo_copy_bytes(void* dst, const void* src, int64_t nbytes, recalgo_stream_t stream) {
    RECALGO_REQUIRE(nbytes >= 0 && (nbytes == 0 || (dst != nullptr && src != nullptr)));
    if (nbytes == 0) return 0;
    size_t head = 0, n16 = 0;
    // same phase: vector body between a byte head and a byte tail (copy_span.h)
    if (!recalgo_copy::copy_span_split(dst, src, (size_t)nbytes, &head, &n16)) {
        // different phase: whole span by the byte lanes (rare: every batch allocation of the library is 256-byte aligned);
        // handled as repeated launches of the byte paths below would be slow, so fall back to the runtime's copy
        return (int)hipMemcpyAsync(dst, src, (size_t)nbytes, hipMemcpyDeviceToDevice, as_stream(stream));
    }
    const unsigned blocks = recalgo_copy::copy_span_blocks(n16);
    hipLaunchKernelGGL(copy_bytes_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), static_cast<unsigned char*>(dst),
                       static_cast<const unsigned char*>(src), head, n16, (size_t)nbytes);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_abi_version(void) { return RECALGO_ABI_VERSION; }
RECALGO_EXPORT const char* recalgo_target_arch(void) { return "gfx950"; }

RECALGO_EXPORT int recalgo_sigmoid_ce_fwd_bwd(const float* logits, const float* labels, int B,
                                              float grad_scale, float* prob, float* loss,
                                              float* dlogit, recalgo_stream_t stream) {
    RECALGO_REQUIRE(B > 0);
    hipLaunchKernelGGL(sigmoid_ce_kernel, dim3(1), dim3(1024), 0, as_stream(stream), logits, labels,
                       (unsigned)B, grad_scale, prob, loss, dlogit);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_adam_tf1_advance(int64_t* step_dev, float lr, float beta1, float beta2,
                                            float* lr_t_dev, recalgo_stream_t stream) {
    RECALGO_REQUIRE(step_dev != nullptr && lr_t_dev != nullptr);
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, as_stream(stream), step_dev, lr, beta1,
                       beta2, lr_t_dev);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_adam_tf1_dense(float* p, float* g, float* m, float* v, int64_t n,
                                          float lr_t, const float* lr_t_dev, float beta1, float beta2,
                                          float eps, int zero_grad, recalgo_stream_t stream) {
    RECALGO_REQUIRE(n >= 0);
    if (n == 0) return 0;
    RECALGO_REQUIRE(aligned16(p, g, m, v));            // (the float4 body; the n % 4 tail is element-wise)
    int64_t n4 = n / 4;
    int64_t want = (n4 + 255) / 256;
    int blocks = (int)(want < 1 ? 1 : (want > 256 * 16 ? 256 * 16 : want));
    hipLaunchKernelGGL(adam_tf1_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), p, g, m, v, n4,
                       n, lr_t, lr_t_dev, beta1, beta2, eps, zero_grad);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_adam_tf1_rows(float* p, float* g, float* m, float* v, unsigned char* row_live,
                                         int64_t rows, int K, float lr_t, const float* lr_t_dev, float beta1,
                                         float beta2, float eps, int zero_grad, recalgo_stream_t stream) {
    RECALGO_REQUIRE(rows >= 0 && row_live != nullptr);
    RECALGO_REQUIRE(K == 4 || K == 8 || K == 16 || K == 32 || K == 64);
    if (rows == 0) return 0;
    RECALGO_REQUIRE(aligned16(p, g, m, v));
    const int64_t total4 = rows * (K / 4);
    int64_t want = (total4 + 255) / 256;
    int blocks = (int)(want < 1 ? 1 : (want > 256 * 16 ? 256 * 16 : want));
    hipStream_t st = as_stream(stream);
#define LAUNCH(KK4)                                                                                       \
    hipLaunchKernelGGL(adam_tf1_rows_kernel<KK4>, dim3(blocks), dim3(256), 0, st, p, g, m, v, row_live, total4, \
                       lr_t, lr_t_dev, beta1, beta2, eps, zero_grad)
    switch (K / 4) {
        case 1: LAUNCH(1); break;
        case 2: LAUNCH(2); break;
        case 4: LAUNCH(4); break;
        case 8: LAUNCH(8); break;
        default: LAUNCH(16); break;
    }
#undef LAUNCH
    RECALGO_RETURN_LAST();
}

// any row width (e.g. the K = 1 first-order weights of DeepFM): one float per thread
__global__ __launch_bounds__(256) void adam_tf1_list_scalar_kernel(float* __restrict__ p, float* __restrict__ g,
                                                                   float* __restrict__ m, float* __restrict__ v,
                                                                   const int* __restrict__ list,
                                                                   const int* __restrict__ count, unsigned K,
                                                                   float lr_t_val, const float* __restrict__ lr_t_dev,
                                                                   float b1, float b2, float eps, int zero_grad) {
    const float lr_t = lr_t_dev ? lr_t_dev[0] : lr_t_val;
    const int64_t total = (int64_t)count[0] * K;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
        const int64_t i = (int64_t)list[t / K] * K + (t % K);
        float gg = g[i], mm = m[i], vv = v[i], pp = p[i];
        const bool nz = gg != 0.f;
        adam1(pp, gg, mm, vv, lr_t, b1, b2, eps);
        p[i] = pp; m[i] = mm; v[i] = vv;
        if (zero_grad && nz) g[i] = 0.f;
    }
}

RECALGO_EXPORT int recalgo_mark_live_rows(const int64_t* ids, const int64_t* row_base, int64_t n, int F,
                                          unsigned char* row_live, int* live_list, int* live_count,
                                          recalgo_stream_t stream) {
    RECALGO_REQUIRE(n >= 0 && F >= 1 && row_live != nullptr && live_list != nullptr && live_count != nullptr);
    RECALGO_REQUIRE((reinterpret_cast<uintptr_t>(row_live) & 3) == 0);
    if (n == 0) return 0;
    hipLaunchKernelGGL(mark_live_rows_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), ids, row_base, n,
                       (unsigned)F, reinterpret_cast<unsigned*>(row_live), live_list, live_count);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int64_t recalgo_order_live_list_workspace_bytes(int64_t rows) {
    const int64_t n_words = (rows + 3) / 4;
    return ((n_words + kChunkWords - 1) / kChunkWords) * (int64_t)sizeof(int);
}

RECALGO_EXPORT int recalgo_order_live_list(const unsigned char* row_live, int64_t rows, int* live_list,
                                           int* live_count, void* workspace, recalgo_stream_t stream) {
    RECALGO_REQUIRE(rows >= 0 && row_live != nullptr && live_list != nullptr && live_count != nullptr);
    RECALGO_REQUIRE((reinterpret_cast<uintptr_t>(row_live) & 3) == 0);
    if (rows == 0) return 0;
    RECALGO_REQUIRE(workspace != nullptr);
    hipStream_t st = as_stream(stream);
    const int64_t n_words = (rows + 3) / 4;
    const int n_chunks = cdiv(n_words, kChunkWords);
    const unsigned* words = reinterpret_cast<const unsigned*>(row_live);
    int* chunk = static_cast<int*>(workspace);
    hipLaunchKernelGGL(live_chunk_count_kernel, dim3(n_chunks), dim3(256), 0, st, words, n_words, chunk);
    hipLaunchKernelGGL(live_chunk_scan_kernel, dim3(1), dim3(1024), 0, st, chunk, n_chunks, live_count);
    hipLaunchKernelGGL(live_chunk_write_kernel, dim3(n_chunks), dim3(256), 0, st, words, n_words, rows, chunk, live_list);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_adam_tf1_list(float* p, float* g, float* m, float* v, const int* live_list,
                                         const int* live_count, int64_t max_rows, int K, float lr_t,
                                         const float* lr_t_dev, float beta1, float beta2, float eps,
                                         int zero_grad, recalgo_stream_t stream) {
    RECALGO_REQUIRE(max_rows >= 0 && K >= 1 && live_list != nullptr && live_count != nullptr);
    if (max_rows == 0) return 0;
    hipStream_t st = as_stream(stream);
    if (!(K == 4 || K == 8 || K == 16 || K == 32 || K == 64)) {
        int64_t want1 = (max_rows * K + 255) / 256;
        int blocks1 = (int)(want1 < 1 ? 1 : (want1 > 256 * 8 ? 256 * 8 : want1));
        hipLaunchKernelGGL(adam_tf1_list_scalar_kernel, dim3(blocks1), dim3(256), 0, st, p, g, m, v, live_list,
                           live_count, (unsigned)K, lr_t, lr_t_dev, beta1, beta2, eps, zero_grad);
        RECALGO_RETURN_LAST();
    }
    RECALGO_REQUIRE(aligned16(p, g, m, v));            // (the float4 kernels; the element-wise one above takes any base)
    // the launch is sized for the largest possible list (graph replayable); surplus workgroups exit at once
    int64_t want = (max_rows * (K / 4) + 255) / 256;
    int blocks = (int)(want < 1 ? 1 : (want > 256 * 8 ? 256 * 8 : want));
#define LAUNCH(KK4)                                                                                         \
    hipLaunchKernelGGL(adam_tf1_list_kernel<KK4>, dim3(blocks), dim3(256), 0, st, p, g, m, v, live_list, live_count, \
                       lr_t, lr_t_dev, beta1, beta2, eps, zero_grad)
    switch (K / 4) {
        case 1: LAUNCH(1); break;
        case 2: LAUNCH(2); break;
        case 4: LAUNCH(4); break;
        case 8: LAUNCH(8); break;
        default: LAUNCH(16); break;
    }
#undef LAUNCH
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_activation_fwd(const float* x, const float* alpha, int rows, int C,
                                          int kind, float* y, recalgo_stream_t stream) {
    RECALGO_REQUIRE(rows >= 0 && C > 0 && (kind == RECALGO_ACT_PRELU || kind == RECALGO_ACT_DICE));
    int64_t n = (int64_t)rows * C;
    if (n == 0) return 0;
    if (kind == RECALGO_ACT_DICE)
        hipLaunchKernelGGL(act_fwd_kernel<true>, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), x,
                           alpha, n, (unsigned)C, y);
    else
        hipLaunchKernelGGL(act_fwd_kernel<false>, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), x,
                           alpha, n, (unsigned)C, y);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int64_t recalgo_activation_bwd_workspace_bytes(int rows, int C) {
    if (rows <= 0 || C <= 0) return 0;
    return (int64_t)cdiv(rows, kActRowsPerBlk) * C * (int64_t)sizeof(float);
}

RECALGO_EXPORT int recalgo_activation_bwd_partial_rows(int rows, int C) {
    if (rows <= 0 || C <= 0) return 0;
    return C % 4 == 0 ? cdiv(rows, kActTileRows) : cdiv(rows, kActRowsPerBlk);
}
RECALGO_EXPORT int recalgo_activation_bwd(const float* x, const float* alpha, const float* gy,
                                          int rows, int C, int kind, float* dx, float* dalpha,
                                          void* workspace, recalgo_stream_t stream) {
    RECALGO_REQUIRE(rows > 0 && C > 0 && workspace != nullptr);
    RECALGO_REQUIRE(kind == RECALGO_ACT_PRELU || kind == RECALGO_ACT_DICE);
    float* partial = static_cast<float*>(workspace);
    hipStream_t st = as_stream(stream);
    if (C % 4 == 0) {
        const unsigned nt = (unsigned)cdiv(rows, kActTileRows), C4 = (unsigned)C / 4;
        const dim3 grid(cdiv(C4, 16), nt);
        if (kind == RECALGO_ACT_DICE)
            hipLaunchKernelGGL(act_bwd_tile_kernel<true>, grid, dim3(256), 0, st, reinterpret_cast<const float4*>(x),
                               reinterpret_cast<const float4*>(alpha), reinterpret_cast<const float4*>(gy),
                               (unsigned)rows, C4, reinterpret_cast<float4*>(dx), reinterpret_cast<float4*>(partial));
        else
            hipLaunchKernelGGL(act_bwd_tile_kernel<false>, grid, dim3(256), 0, st, reinterpret_cast<const float4*>(x),
                               reinterpret_cast<const float4*>(alpha), reinterpret_cast<const float4*>(gy),
                               (unsigned)rows, C4, reinterpret_cast<float4*>(dx), reinterpret_cast<float4*>(partial));
        if (dalpha) launch_colsum16(partial, nt, (unsigned)C, dalpha, (unsigned)C, static_cast<float*>(nullptr), st);
        RECALGO_RETURN_LAST();
    }
    const unsigned nblk = (unsigned)cdiv(rows, kActRowsPerBlk);
    if (kind == RECALGO_ACT_DICE)
        hipLaunchKernelGGL(act_bwd_kernel<true>, dim3(nblk), dim3(256), 0, st, x, alpha, gy, (unsigned)rows,
                           (unsigned)C, kActRowsPerBlk, dx, partial);
    else
        hipLaunchKernelGGL(act_bwd_kernel<false>, dim3(nblk), dim3(256), 0, st, x, alpha, gy, (unsigned)rows,
                           (unsigned)C, kActRowsPerBlk, dx, partial);
    if (dalpha) launch_colsum16(partial, nblk, (unsigned)C, dalpha, (unsigned)C, static_cast<float*>(nullptr), st);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_adam_tf1_step(float* p, float* g, float* m, float* v, int64_t n,
                                         const recalgo_adam_arena_t* arenas, int n_arenas, int64_t* step_dev,
                                         int* ticket_dev, int advance, float lr, float beta1, float beta2, float eps,
                                         int zero_grad, recalgo_stream_t stream) {
    return recalgo_adam_tf1_step_plans(p, g, m, v, n, arenas, n_arenas, step_dev, ticket_dev, advance, lr, beta1, beta2, eps,
                                       zero_grad, nullptr, 0, stream);
}

// The launch's arguments but for the dense workgroups (A.dense_blocks: set by the caller, who launches A.scan_first + n_scans
// workgroups) -> 0 or hipErrorInvalidValue
static int fill_adam_step_args(AdamStepArgs& A, float* p, float* g, float* m, float* v, int64_t n, const recalgo_adam_arena_t* arenas,
                               int n_arenas, int64_t* step_dev, int* ticket_dev, int advance, float lr, float beta1, float beta2,
                               float eps, int zero_grad, const recalgo_plan_scan_t* scans, int n_scans) {
    RECALGO_REQUIRE(n >= 0 && n_arenas >= 0 && n_arenas <= kAdamMaxArenas && step_dev != nullptr);
    RECALGO_REQUIRE(n_scans >= 0 && n_scans <= kAdamMaxArenas && (n_scans == 0 || scans != nullptr));
    RECALGO_REQUIRE(!advance || ticket_dev != nullptr);
    RECALGO_REQUIRE(n == 0 || (p && g && m && v && aligned16(p, g, m, v)));
    RECALGO_REQUIRE(n_arenas == 0 || arenas != nullptr);
    A.p = p; A.g = g; A.m = m; A.v = v; A.n = n;
    unsigned blocks = A.dense_blocks;
    A.n_arenas = 0;
    for (int i = 0; i < n_arenas; ++i) {
        const recalgo_adam_arena_t& a = arenas[i];
        if (a.max_rows <= 0) continue;
        RECALGO_REQUIRE(a.p && a.g && a.m && a.v && a.live_list && a.live_count && a.K >= 1);
        RECALGO_REQUIRE((a.K & 3) != 0 || aligned16(a.p, a.g, a.m, a.v));      // (the float4 arms)
        AdamArena& R = A.ar[A.n_arenas++];
        R.p = a.p; R.g = a.g; R.m = a.m; R.v = a.v; R.list = a.live_list; R.count = a.live_count; R.K = a.K;
        R.k4_shift = -1;
        R.lazy = a.lazy;
        if ((a.K & 3) == 0)
            for (int sft = 0; sft < 16; ++sft)
                if ((a.K >> 2) == (1 << sft)) R.k4_shift = sft;
        // the lazy vote of this (live-list) path is per row only when the K/4 lanes of a row are an aligned power-of-two
        // group of one wave; other widths would vote per float4 / per element, which is not LazyAdam (the owner-computes
        // path, recalgo_scatter_apply RECALGO_SCATTER_LAZY_ADAM, has no such limit and is what the host uses)
        RECALGO_REQUIRE(!a.lazy || (R.k4_shift >= 0 && (a.K >> 2) <= 64));
        // sized for the largest possible list (graph replayable); surplus workgroups find nothing to do
        const int64_t per = (a.K & 3) == 0 ? a.max_rows * (a.K / 4) : a.max_rows * a.K;
        const int64_t w = (per + 255) / 256;
        R.n_blocks = (unsigned)(w < 1 ? 1 : (w > 2048 ? 2048 : w));
        R.first_block = blocks;
        blocks += R.n_blocks;
    }
    for (int i = A.n_arenas; i < kAdamMaxArenas; ++i) A.ar[i] = AdamArena{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 4, 0, 0, 0xffffffffu, 0};
    A.step = reinterpret_cast<long long*>(step_dev); A.ticket = ticket_dev; A.advance = advance;
    A.lr = lr; A.b1 = beta1; A.b2 = beta2; A.eps = eps; A.zero_grad = zero_grad;
    if (blocks == 0) blocks = 1;                      // still advances the step counter
    A.scan_first = blocks;
    for (int i = 0; i < n_scans; ++i) {
        const recalgo_plan_scan_t& c = scans[i];
        RECALGO_REQUIRE(c.total && c.offs && c.sched && c.nb_log2 >= 8 && c.nb_log2 <= 13 && c.counter_shift <= 5);
        A.scan[i] = recalgo_plan::Scan{c.total, c.offs, static_cast<uint4*>(c.sched), c.counter_shift, c.nb_log2};
    }
    for (int i = n_scans; i < kAdamMaxArenas; ++i) A.scan[i] = recalgo_plan::Scan{nullptr, nullptr, nullptr, 0, 8};
    return 0;
}

RECALGO_EXPORT int recalgo_adam_tf1_step_plans(float* p, float* g, float* m, float* v, int64_t n,
                                               const recalgo_adam_arena_t* arenas, int n_arenas, int64_t* step_dev,
                                               int* ticket_dev, int advance, float lr, float beta1, float beta2, float eps,
                                               int zero_grad, const recalgo_plan_scan_t* scans, int n_scans,
                                               recalgo_stream_t stream) {
    RECALGO_REQUIRE(n >= 0);
    AdamStepArgs A;
    const int64_t want = (n / 4 + 255) / 256;
    A.dense_blocks = n == 0 ? 0u : (unsigned)(want < 1 ? 1 : (want > 4096 ? 4096 : want));
    const int rc = fill_adam_step_args(A, p, g, m, v, n, arenas, n_arenas, step_dev, ticket_dev, advance, lr, beta1, beta2, eps,
                                       zero_grad, scans, n_scans);
    if (rc) return rc;
    hipLaunchKernelGGL(adam_tf1_step_kernel, dim3(A.scan_first + (unsigned)n_scans), dim3(256), 0, as_stream(stream), A);
    RECALGO_RETURN_LAST();
}

// The job table of the sum-and-step launch and the intervals of the flat buffer no job writes -> 1, or 0 where the launch cannot
// serve the jobs (recalgo_adam_tf1_sum_step_supported)
static int build_sum_step(SumStepArgs& K, const float* g, int64_t n, const recalgo_dense_split_t* jobs, int n_jobs,
                          const recalgo_colsum_t* sums, int n_sums, const recalgo_colsum_t* side_sums, int n_side_sums) {
    if (n < 0 || n_jobs < 0 || n_sums < 0 || n_side_sums < 0 || (n_jobs && !jobs) || (n_sums && !sums) || (n_side_sums && !side_sums))
        return 0;
    if (n > 0 && (g == nullptr || !aligned16(g))) return 0;
    std::vector<recalgo_colsum_t> cs(sums, sums + n_sums);
    cs.insert(cs.end(), side_sums, side_sums + n_side_sums);
    unsigned blocks = 0;
    if (recalgo_build_split_jobs(jobs, n_jobs, cs.data(), (int)cs.size(), K.job, kSumStepMaxJobs, &K.n_jobs, &blocks) != 0) return 0;
    K.job_blocks = blocks;
    const uintptr_t g0 = reinterpret_cast<uintptr_t>(g), g1 = g0 + (uintptr_t)n * sizeof(float);
    std::vector<std::pair<int64_t, int64_t>> outs;               // [lo, hi) in elements of the flat buffer
    for (int j = 0; j < K.n_jobs; ++j) {
        const recalgo_slabs::SplitJob& jb = K.job[j];
        const bool side = jb.vec == 2 && j >= n_sums;            // (the column sums come first, in the caller's order)
        const std::pair<const float*, unsigned long long> o[2] = {{jb.out0, jb.n0}, {jb.out1, jb.n - jb.n0}};
        for (int h = 0; h < 2; ++h) {
            if (o[h].second == 0) continue;
            const uintptr_t a = reinterpret_cast<uintptr_t>(o[h].first), b = a + (uintptr_t)o[h].second * sizeof(float);
            if (side) {
                if (a < g1 && b > g0) return 0;                    // a value that is no gradient, inside the gradient buffer
                continue;
            }
            if (a < g0 || b > g1 || (a - g0) % sizeof(float) != 0) return 0;
            // (the float4 path's outputs are 16-byte aligned, as is g: make_split_job)
            outs.emplace_back((int64_t)((a - g0) / sizeof(float)), (int64_t)((b - g0) / sizeof(float)));
        }
    }
    std::sort(outs.begin(), outs.end());
    K.n_rest = 0;
    int64_t at = 0, rest = 0;
    auto gap = [&](int64_t lo, int64_t hi) {
        if (lo >= hi) return;
        K.rest_lo[K.n_rest] = lo; K.rest_hi[K.n_rest] = hi;
        ++K.n_rest;
        rest += hi - lo;
    };
    for (const auto& o : outs) {
        if (o.first < at) return 0;                                // two outputs overlap
        gap(at, o.first);
        at = o.second;
    }
    gap(at, n);
    const int64_t want = (rest / 4 + 255) / 256;
    K.rest_blocks = rest == 0 ? 0u : (unsigned)(want < 1 ? 1 : (want > 4096 ? 4096 : want));
    return 1;
}

RECALGO_EXPORT int64_t recalgo_adam_tf1_sum_step_workspace_bytes(void) { return (int64_t)kTicketInts * (int64_t)sizeof(int); }

// (include/recalgo_sumstep.h declares the descriptor arrays of recalgo.h as const void*: that header stands alone)
RECALGO_EXPORT int recalgo_sumstep_abi_version(void) { return RECALGO_SUMSTEP_ABI_VERSION; }

RECALGO_EXPORT int recalgo_adam_tf1_sum_step_supported(const float* g, int64_t n, const void* jobs, int n_jobs, const void* sums,
                                                       int n_sums, const void* side_sums, int n_side_sums) {
    SumStepArgs K;
    return build_sum_step(K, g, n, static_cast<const recalgo_dense_split_t*>(jobs), n_jobs, static_cast<const recalgo_colsum_t*>(sums),
                          n_sums, static_cast<const recalgo_colsum_t*>(side_sums), n_side_sums);
}

RECALGO_EXPORT int recalgo_adam_tf1_sum_step(float* p, float* g, float* m, float* v, int64_t n, const void* arenas_, int n_arenas,
                                             int64_t* step_dev, int* ticket_dev, int advance, float lr, float beta1, float beta2,
                                             float eps, int zero_grad, const void* scans_, int n_scans, const void* jobs, int n_jobs,
                                             const void* sums, int n_sums, const void* side_sums, int n_side_sums,
                                             recalgo_stream_t stream) {
    const recalgo_adam_arena_t* arenas = static_cast<const recalgo_adam_arena_t*>(arenas_);
    const recalgo_plan_scan_t* scans = static_cast<const recalgo_plan_scan_t*>(scans_);
    SumStepArgs K;
    RECALGO_REQUIRE(build_sum_step(K, g, n, static_cast<const recalgo_dense_split_t*>(jobs), n_jobs,
                                   static_cast<const recalgo_colsum_t*>(sums), n_sums, static_cast<const recalgo_colsum_t*>(side_sums),
                                   n_side_sums));
    for (int j = K.n_jobs; j < kSumStepMaxJobs; ++j) K.job[j] = recalgo_slabs::SplitJob{nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0xffffffffu};
    for (int k = K.n_rest; k < kSumStepMaxRest; ++k) K.rest_lo[k] = K.rest_hi[k] = 0;
    K.A.dense_blocks = K.job_blocks + K.rest_blocks;
    const int rc = fill_adam_step_args(K.A, p, g, m, v, n, arenas, n_arenas, step_dev, ticket_dev, advance, lr, beta1, beta2, eps,
                                       zero_grad, scans, n_scans);
    if (rc) return rc;
    K.lr_block = ticket_dev != nullptr ? K.A.scan_first + (unsigned)n_scans : 0xffffffffu;
    hipLaunchKernelGGL(sums_adam_tf1_step_kernel, dim3(K.A.scan_first + (unsigned)n_scans + (ticket_dev != nullptr ? 1u : 0u)), dim3(256),
                       0, as_stream(stream), K);
    RECALGO_RETURN_LAST();
}
