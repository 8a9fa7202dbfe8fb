// FFM's field-aware second-order term (include/recalgo_ffm.h; /root/reference algorithm/FFM/ffm.py:146-160) without its operand
// tensor.  X [B, F (F - 1) K] of the composed path (gather -> recalgo_ffm_pairs_*) holds every looked-up row once and every
// element of it belongs to exactly one pair, so nothing is reused: the forward fetches the two rows of a pair and dots them,
// the backward fetches a request's partner row again and scales it by g[b].  Both are gather kernels and memory-bound:
//   * a wave serves an example; a lane owns one 16-byte piece of a row at a time, so the KV = K / 4 lanes of a row read it as
//     one contiguous 4 K bytes, and the loop over a wave's items is unrolled: several rows in flight per lane;
//   * what a lane indexes by a value of its own — the fields' row bases and vocabularies, the example's ids, the pair table —
//     is in LDS: the descriptors arrive as kernel arguments and are copied there once per workgroup;
//   * a bag field's row is the mean over the bag's kept entries, summed in bag order by the lane that needs the piece (the
//     reference's bags hold 0 .. 5 values);
//   * the backward writes each gradient row once, in the layout the scatter's sources read: [B, n_single (F - 1) K] for the
//     single-valued requests (a wave's stores are contiguous) and [capacity, (F - 1) K] per bag field, whose entries outside
//     every bag are zeroed by further workgroups of the same grid.
// The de-duplication of a bag (utils.py:49-64) is one launch over fixed shapes: a thread per entry and a thread per bag.
#include "common.h"
#include "deferred.h"
#include "../../include/recalgo_ffm.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxF = RECALGO_FFM_MAX_F, kMaxBags = RECALGO_FFM_MAX_BAGS;
constexpr int kMaxPairs = kMaxF * (kMaxF - 1) / 2;
constexpr unsigned kTailPieces = 8;          // 16-byte pieces per thread of a workgroup that zeroes the tail of a bag's rows

struct Bag {
    const int64_t* values;
    const int64_t* offsets;
    const int32_t* distinct;
    float* d_rows;
    int capacity;
    unsigned tail0;                          // backward: the first of the bag's tail workgroups, counted from the first of all
};
struct Params {
    long long row_base[kMaxF];
    long long vocab[kMaxF];
    Bag bags[kMaxBags];
    signed char bag[kMaxF];                  // < 0: single-valued
    unsigned char col[kMaxF];                // single-valued field -> its column of ids
    unsigned char sfield[kMaxF];             // column of ids -> field
    unsigned char bfield[kMaxBags];          // bag -> field
    int n_bags, n_single;
};
static_assert(sizeof(Params) % 4 == 0, "copied to LDS as 32-bit words");

// what a wave keeps of its example
struct Example {
    long long base[kMaxF];                   // single-valued field: row_base + id, or -1 (OOV)
    int lo[kMaxBags], hi[kMaxBags], distinct[kMaxBags];
};

__device__ __forceinline__ void load_params(Params& sp, const Params& P) {
    const int* src = reinterpret_cast<const int*>(&P);
    int* dst = reinterpret_cast<int*>(&sp);
    for (unsigned i = threadIdx.x; i < sizeof(Params) / 4; i += kThreads) dst[i] = src[i];
}

__device__ __forceinline__ void load_example(const Params& sp, Example& ex, const int64_t* __restrict__ ids, unsigned b, unsigned F,
                                             unsigned lane) {
    if (lane < F) {
        long long r = -1;
        if (sp.bag[lane] < 0) {
            const long long id = ids[(size_t)b * sp.n_single + sp.col[lane]];
            if (id >= 0) r = sp.row_base[lane] + id;
        }
        ex.base[lane] = r;
    }
    if (lane < (unsigned)sp.n_bags) {
        const Bag& g = sp.bags[lane];
        const long long cap = g.capacity;
        const long long lo = min(max((long long)g.offsets[b], 0ll), cap);
        ex.lo[lane] = (int)lo;
        ex.hi[lane] = (int)min(max((long long)g.offsets[b + 1], lo), cap);
        ex.distinct[lane] = g.distinct[b];
    }
}

// piece q of v_f[s] of the wave's example
template <bool BAGS, bool VIEW>
__device__ __forceinline__ float4 fetch(const Params& sp, const Example& ex, const float4* __restrict__ arena, unsigned f, unsigned s,
                                        unsigned q, unsigned KV, const recalgo_deferred::ReadView& D) {
    const long long sub = (long long)s * sp.vocab[f];
    const int k = BAGS ? sp.bag[f] : -1;
    if (k < 0) {
        // (an OOV id reads row 0 and drops it: the load does not hang on a branch, so the loads of an unrolled loop go out together)
        const long long r0 = ex.base[f];
        const bool ok = r0 >= 0;
        const long long row = ok ? r0 + sub : 0;
        float4 w = arena[(size_t)row * KV + q];
        if (VIEW && ok) w = recalgo_deferred::current_piece(D, w, row, q, KV);
        return ok ? w : f4_zero();
    }
    const int d = ex.distinct[k];
    float4 acc = f4_zero();
    if (d <= 0) return acc;
    const int64_t* __restrict__ vals = sp.bags[k].values;
    const long long rb = sp.row_base[f] + sub;
    for (int e = ex.lo[k]; e < ex.hi[k]; ++e) {
        const long long id = vals[e];
        if (id < 0) continue;
        const long long row = rb + id;
        float4 w = arena[(size_t)row * KV + q];
        if (VIEW) w = recalgo_deferred::current_piece(D, w, row, q, KV);
        acc = f4_add(acc, w);
    }
    const float c = (float)d;
    return make_float4(__fdiv_rn(acc.x, c), __fdiv_rn(acc.y, c), __fdiv_rn(acc.z, c), __fdiv_rn(acc.w, c));
}

template <bool BAGS, bool VIEW>
__global__ __launch_bounds__(kThreads) void ffm_fwd_kernel(const int64_t* __restrict__ ids, const Params P,
                                                           const float4* __restrict__ arena, unsigned B, unsigned F, unsigned KV,
                                                           float* __restrict__ out, const recalgo_deferred::ReadView D) {
    __shared__ Params sp;
    __shared__ Example exs[kWaves];
    __shared__ unsigned short pij[kMaxPairs];                // pair p, row-major over the strict upper triangle -> i << 8 | j
    load_params(sp, P);
    const unsigned NP = F * (F - 1) / 2;
    for (unsigned p = threadIdx.x; p < NP; p += kThreads) {
        unsigned i = 0, rem = p;
        while (rem >= F - 1 - i) { rem -= F - 1 - i; ++i; }
        pij[p] = (unsigned short)(i << 8 | (i + 1 + rem));
    }
    __syncthreads();
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    Example& ex = exs[wave];
    // item t = p * KV + q of a lane advances by 64 per round: (p, q) as a counter with carry, no division in the loop
    const unsigned dp = 64 / KV, dq = 64 % KV;
    for (unsigned b = blockIdx.x * kWaves + wave; b < B; b += gridDim.x * kWaves) {
        load_example(sp, ex, ids, b, F, lane);
        wave_sync();
        float acc = 0.f;
        unsigned p = lane / KV, q = lane % KV;
#pragma unroll 4
        for (; p < NP; p += dp) {
            const unsigned ij = pij[p], i = ij >> 8, j = ij & 255;
            const float4 a = fetch<BAGS, VIEW>(sp, ex, arena, i, j - 1, q, KV, D);
            const float4 c = fetch<BAGS, VIEW>(sp, ex, arena, j, i, q, KV, D);
            acc += f4_dot(a, c);
            q += dq;
            if (q >= KV) { q -= KV; ++p; }
        }
        acc = wave_sum(acc);
        if (lane == 0) out[b] = acc;
        wave_sync();                                         // (the next example overwrites ex)
    }
}

// element (a, s) belongs to exactly one pair: its partner is (s + 1, a) when s >= a, (s, a - 1) when s < a
template <bool BAGS>
__global__ __launch_bounds__(kThreads) void ffm_bwd_kernel(const float* __restrict__ g, const int64_t* __restrict__ ids, const Params P,
                                                           const float4* __restrict__ arena, unsigned B, unsigned F, unsigned KV,
                                                           float4* __restrict__ d_single, unsigned ex_blocks) {
    __shared__ Params sp;
    __shared__ Example exs[kWaves];
    load_params(sp, P);
    __syncthreads();
    const recalgo_deferred::ReadView D{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0.f, 0.f, 0.f, 0};
    const unsigned FS = F - 1, RP = FS * KV;                  // 16-byte pieces of a field's F - 1 gradient rows
    if (BAGS && blockIdx.x >= ex_blocks) {
        // the entries of a bag's buffer that belong to no bag: zeros
        const unsigned tb = blockIdx.x - ex_blocks;
        int k = 0;
        while (k + 1 < sp.n_bags && tb >= sp.bags[k + 1].tail0) ++k;
        const Bag& bg = sp.bags[k];
        const long long cap = bg.capacity;
        const long long first = min(max((long long)bg.offsets[0], 0ll), cap), nnz = min(max((long long)bg.offsets[B], first), cap);
        const size_t total = (size_t)cap * RP;
        size_t i = (size_t)(tb - bg.tail0) * (kThreads * kTailPieces) + threadIdx.x;
        for (unsigned u = 0; u < kTailPieces && i < total; ++u, i += kThreads) {
            const long long e = (long long)(i / RP);
            if (e < first || e >= nnz) reinterpret_cast<float4*>(bg.d_rows)[i] = f4_zero();
        }
        return;
    }
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    Example& ex = exs[wave];
    const unsigned total1 = (unsigned)sp.n_single * RP;
    // item t = (a' * FS + s) * KV + q advances by 64 per round: (a', s, q) as a counter with carries
    const unsigned da = 64 / RP, ds = (64 % RP) / KV, dq = 64 % KV;
    for (unsigned b = blockIdx.x * kWaves + wave; b < B; b += ex_blocks * kWaves) {
        load_example(sp, ex, ids, b, F, lane);
        wave_sync();
        const float gb = g[b];
        float4* __restrict__ row = d_single + (size_t)b * total1;
        unsigned ac = lane / RP, s = (lane % RP) / KV, q = lane % KV;
#pragma unroll 4
        for (unsigned t = lane; t < total1; t += 64) {
            const unsigned a = sp.sfield[ac];
            const unsigned pa = s >= a ? s + 1 : s, ps = s >= a ? a : a - 1;
            row[t] = f4_scale(fetch<BAGS, false>(sp, ex, arena, pa, ps, q, KV, D), gb);
            q += dq;
            if (q >= KV) { q -= KV; ++s; }
            s += ds;
            if (s >= FS) { s -= FS; ++ac; }
            ac += da;
        }
        if (BAGS) {
            for (int k = 0; k < sp.n_bags; ++k) {
                const int lo = ex.lo[k], hi = ex.hi[k], d = ex.distinct[k];
                if (lo >= hi) continue;
                const unsigned a = sp.bfield[k];
                const float c = d > 0 ? __fdiv_rn(gb, (float)d) : 0.f;
                const int64_t* __restrict__ vals = sp.bags[k].values;
                float4* __restrict__ rows = reinterpret_cast<float4*>(sp.bags[k].d_rows);
                for (unsigned t = lane; t < RP; t += 64) {
                    const unsigned s2 = t / KV, q2 = t - s2 * KV;
                    const unsigned pa = s2 >= a ? s2 + 1 : s2, ps = s2 >= a ? a : a - 1;
                    const float4 v = d > 0 ? f4_scale(fetch<BAGS, false>(sp, ex, arena, pa, ps, q2, KV, D), c) : f4_zero();
                    for (int e = lo; e < hi; ++e) rows[(size_t)e * RP + t] = vals[e] >= 0 ? v : f4_zero();
                }
            }
        }
        wave_sync();
    }
}

// the bag of entry j < nnz: the number of bag ends at or before j (as recalgo_bag_mean_grad_rows finds it)
__device__ __forceinline__ int bag_of(const int64_t* __restrict__ offsets, int B, long long j) {
    int lo = 0, hi = B;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (offsets[1 + mid] <= j) lo = mid + 1;
        else hi = mid;
    }
    return min(lo, B - 1);
}

// thread t < n: entry t; thread n + b: the counts of bag b
__global__ __launch_bounds__(kThreads) void ffm_bag_distinct_kernel(const int64_t* __restrict__ values, const int64_t* __restrict__ offsets,
                                                                    int B, long long n, int64_t* __restrict__ out_values,
                                                                    int32_t* __restrict__ valid, int32_t* __restrict__ distinct) {
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long nnz = min(max((long long)offsets[B], 0ll), n);
    if (t < n) {
        long long keep = -1;
        if (t < nnz) {
            const long long id = values[t];
            if (id >= 0) {
                const int b = bag_of(offsets, B, t);
                bool seen = false;
                for (long long e = max((long long)offsets[b], 0ll); e < t && !seen; ++e) seen = values[e] == id;
                if (!seen) keep = id;
            }
        }
        out_values[t] = keep;
    } else if (t < n + B) {
        const int b = (int)(t - n);
        const long long lo = min(max((long long)offsets[b], 0ll), nnz), hi = min(max((long long)offsets[b + 1], lo), nnz);
        int nv = 0, nd = 0;
        for (long long e = lo; e < hi; ++e) {
            const long long id = values[e];
            if (id < 0) continue;
            ++nv;
            bool seen = false;
            for (long long e2 = lo; e2 < e && !seen; ++e2) seen = values[e2] == id;
            nd += seen ? 0 : 1;
        }
        valid[b] = nv;
        distinct[b] = nd;
    }
}

// the descriptors of a call, checked and packed; false: the call is refused
bool pack(const recalgo_ffm_field_t* fields, const recalgo_ffm_bag_t* bags, int n_bags, int F, int K, bool backward, Params* out) {
    if (!recalgo_ffm_supported(F, K, n_bags) || fields == nullptr || (n_bags > 0 && bags == nullptr)) return false;
    Params& P = *out;
    P = Params{};
    P.n_bags = n_bags;
    bool taken[kMaxBags] = {};
    for (int f = 0; f < F; ++f) {
        const recalgo_ffm_field_t& fd = fields[f];
        if (fd.vocab < 1 || fd.row_base < 0) return false;
        P.row_base[f] = fd.row_base;
        P.vocab[f] = fd.vocab;
        if (fd.bag < 0) {
            P.bag[f] = -1;
            P.col[f] = (unsigned char)P.n_single;
            P.sfield[P.n_single++] = (unsigned char)f;
        } else {
            if (fd.bag >= n_bags || taken[fd.bag]) return false;
            taken[fd.bag] = true;
            P.bag[f] = (signed char)fd.bag;
            P.bfield[fd.bag] = (unsigned char)f;
        }
    }
    if (P.n_single != F - n_bags) return false;              // (every bag is named by a field)
    for (int k = 0; k < n_bags; ++k) {
        const recalgo_ffm_bag_t& bg = bags[k];
        if (bg.offsets == nullptr || bg.distinct == nullptr || bg.capacity < 0 || bg.capacity >= (1ll << 31)) return false;
        if (bg.capacity > 0 && (bg.values == nullptr || (backward && bg.d_rows == nullptr))) return false;
        if (!aligned_to<8>(bg.values, bg.offsets) || !aligned_to<4>(bg.distinct) || (backward && !aligned16(bg.d_rows))) return false;
        P.bags[k] = Bag{bg.values, bg.offsets, bg.distinct, backward ? bg.d_rows : nullptr, (int)bg.capacity, 0u};
    }
    return true;
}

}  // namespace

RECALGO_EXPORT int recalgo_ffm_abi_version(void) { return RECALGO_FFM_ABI_VERSION; }

RECALGO_EXPORT int recalgo_ffm_supported(int F, int K, int n_bags) {
    return F >= RECALGO_FFM_MIN_F && F <= RECALGO_FFM_MAX_F && K >= RECALGO_FFM_MIN_K && K <= RECALGO_FFM_MAX_K && K % 4 == 0 &&
                   n_bags >= 0 && n_bags <= RECALGO_FFM_MAX_BAGS && n_bags <= F
               ? 1
               : 0;
}

RECALGO_EXPORT int recalgo_ffm_bag_distinct(const int64_t* values, const int64_t* offsets, int B, int64_t n, int64_t* out_values,
                                            int32_t* valid, int32_t* distinct, recalgo_stream_t stream) {
    RECALGO_REQUIRE(B > 0 && n >= 0 && (int64_t)B + n < (1ll << 31) && offsets && valid && distinct);
    RECALGO_REQUIRE(n == 0 || (values && out_values && values != out_values));
    RECALGO_REQUIRE(aligned_to<8>(values, offsets, out_values) && aligned_to<4>(valid, distinct));
    hipLaunchKernelGGL(ffm_bag_distinct_kernel, dim3(cdiv((int64_t)B + n, kThreads)), dim3(kThreads), 0, as_stream(stream), values,
                       offsets, B, (long long)n, out_values, valid, distinct);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_ffm_fwd(const int64_t* ids, const recalgo_ffm_field_t* fields, const recalgo_ffm_bag_t* bags, int n_bags,
                                   const float* arena, int B, int F, int K, float* out, const void* deferred, const int64_t* step_dev,
                                   int step_offset, recalgo_stream_t stream) {
    Params P;
    RECALGO_REQUIRE(pack(fields, bags, n_bags, F, K, false, &P));
    RECALGO_REQUIRE(B > 0 && arena && out && (ids || P.n_single == 0));
    RECALGO_REQUIRE(aligned_to<8>(ids, step_dev) && aligned16(arena) && aligned_to<4>(out));
    RECALGO_REQUIRE((int64_t)B * P.n_single * (F - 1) * (K / 4) < (1ll << 31));
    const auto* d = static_cast<const recalgo_deferred_adam_t*>(deferred);
    const bool view = d && d->last_step && step_dev;
    RECALGO_REQUIRE(!view || (d->m && d->v && d->lr_ring));
    const recalgo_deferred::ReadView D =
        view ? recalgo_deferred::ReadView{d->m, d->v, d->last_step, d->lr_ring, reinterpret_cast<const long long*>(step_dev), step_offset,
                                          d->beta1, d->beta2, d->eps, 0}
             : recalgo_deferred::ReadView{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0.f, 0.f, 0.f, 0};
    auto* const kernel = n_bags ? (view ? ffm_fwd_kernel<true, true> : ffm_fwd_kernel<true, false>)
                                : (view ? ffm_fwd_kernel<false, true> : ffm_fwd_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(cdiv(B, kWaves)), dim3(kThreads), 0, as_stream(stream), ids, P,
                       reinterpret_cast<const float4*>(arena), (unsigned)B, (unsigned)F, (unsigned)(K / 4), out, D);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_ffm_bwd(const float* g, const int64_t* ids, const recalgo_ffm_field_t* fields, const recalgo_ffm_bag_t* bags,
                                   int n_bags, const float* arena, int B, int F, int K, float* d_single, recalgo_stream_t stream) {
    Params P;
    RECALGO_REQUIRE(pack(fields, bags, n_bags, F, K, true, &P));
    RECALGO_REQUIRE(B > 0 && arena && g && ((ids && d_single) || P.n_single == 0));
    RECALGO_REQUIRE(aligned_to<8>(ids) && aligned16(arena, d_single) && aligned_to<4>(g));
    const int64_t RP = (int64_t)(F - 1) * (K / 4);
    RECALGO_REQUIRE((int64_t)B * P.n_single * RP < (1ll << 31));
    const unsigned ex_blocks = (unsigned)cdiv(B, kWaves);
    int64_t blocks = ex_blocks;
    for (int k = 0; k < n_bags; ++k) {
        P.bags[k].tail0 = (unsigned)(blocks - ex_blocks);
        blocks += cdiv((int64_t)P.bags[k].capacity * RP, (int64_t)kThreads * kTailPieces);
    }
    RECALGO_REQUIRE(blocks < (1ll << 31));
    auto* const kernel = n_bags ? ffm_bwd_kernel<true> : ffm_bwd_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), 0, as_stream(stream), g, ids, P,
                       reinterpret_cast<const float4*>(arena), (unsigned)B, (unsigned)F, (unsigned)(K / 4),
                       reinterpret_cast<float4*>(d_single), ex_blocks);
    RECALGO_RETURN_LAST();
}
