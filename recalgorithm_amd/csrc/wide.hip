// The wide part of Wide&Deep (include/recalgo_wide.h): crossed-column hash + indicator + one-unit dense forward, and the
// deterministic per-bucket gradient sum fused with FTRL.  64-bit integer ALU work and gathers; work proportional to the
// batch's requests (the one exception, by design: the hash_bucket_size-wide zeroing of the first FTRL step).
#include "common.h"

#include "../../include/recalgo_wide.h"

RECALGO_EXPORT int recalgo_wide_abi_version(void) { return RECALGO_WIDE_ABI_VERSION; }

namespace {

constexpr int kThreads = 256;

// workspace: [ header: 4 x int32 (n, total, 0, 0) | bucket[cap] | example[cap] | slot[cap] | seg[cap] | vals[cap] ]
struct WideWs {
    int32_t* hdr;
    int32_t* bucket;
    int32_t* example;
    int32_t* slot;
    int32_t* seg;
    float* vals;
};

__host__ __device__ inline WideWs wide_ws(void* ws, int capacity) {
    WideWs w;
    w.hdr = static_cast<int32_t*>(ws);
    w.bucket = w.hdr + 4;
    w.example = w.bucket + capacity;
    w.slot = w.example + capacity;
    w.seg = w.slot + capacity;
    w.vals = reinterpret_cast<float*>(w.seg + capacity);
    return w;
}

__device__ __forceinline__ uint64_t shift_mix(uint64_t v) { return v ^ (v >> 47); }

// FingerprintCat64
__device__ __forceinline__ uint64_t fingerprint_cat(uint64_t a, uint64_t b) {
    const uint64_t kMul = 0xc6a4a7935bd1e995ULL;
    uint64_t r = a ^ kMul;
    r ^= shift_mix(b * kMul) * kMul;
    r *= kMul;
    r = shift_mix(r) * kMul;
    return shift_mix(r);
}

__device__ __forceinline__ int64_t clamp_i64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one thread per example: its bag's buckets, the counts (TRAIN) and the logit
__global__ __launch_bounds__(kThreads) void wide_fwd_kernel(const int64_t* __restrict__ user_ids, int64_t user_stride,
                                                            const int64_t* __restrict__ tag_values,
                                                            const int64_t* __restrict__ tag_offsets, int64_t tag_stride, int B,
                                                            int capacity, uint64_t H, uint64_t hash_key,
                                                            const float* __restrict__ kernel, const float* __restrict__ bias,
                                                            WideWs w, int32_t* __restrict__ count,
                                                            float* __restrict__ wide_logit) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b == 0) {
        const int64_t n = tag_offsets ? clamp_i64(tag_offsets[B], 0, capacity) : (int64_t)B;
        w.hdr[0] = (int32_t)n;
        w.hdr[1] = 0;
    }
    if (b >= B) return;
    int64_t r0, r1;
    if (tag_offsets) {
        r0 = clamp_i64(tag_offsets[b], 0, capacity);
        r1 = clamp_i64(tag_offsets[b + 1], r0, capacity);
    } else {
        r0 = b;
        r1 = b + 1;
    }
    const uint64_t hu = fingerprint_cat(hash_key, (uint64_t)user_ids[(int64_t)b * user_stride]);
    float acc = 0.f;
    for (int64_t r = r0; r < r1; ++r) {
        const uint64_t t = (uint64_t)tag_values[tag_offsets ? r : r * tag_stride];
        const int32_t j = (int32_t)(fingerprint_cat(hu, t) % H);
        w.bucket[r] = j;
        w.example[r] = b;
        if (count) w.slot[r] = atomicAdd(&count[j], 1);
        acc += kernel[j];
    }
    wide_logit[b] = (bias ? bias[0] : 0.f) + acc;
}

// the first request a bucket's count handed out allocates the bucket's segment
__global__ __launch_bounds__(kThreads) void wide_alloc_kernel(WideWs w, int32_t* __restrict__ count, int32_t* __restrict__ start) {
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= w.hdr[0] || w.slot[r] != 0) return;
    const int32_t j = w.bucket[r];
    start[j] = atomicAdd(&w.hdr[1], count[j]);
}

__global__ __launch_bounds__(kThreads) void wide_place_kernel(WideWs w, const int32_t* __restrict__ start) {
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= w.hdr[0]) return;
    w.seg[start[w.bucket[r]] + w.slot[r]] = r;
}

// rank of r among its bucket's request indices -> the place of its gradient term in the segment
__global__ __launch_bounds__(kThreads) void wide_rank_kernel(WideWs w, const int32_t* __restrict__ count,
                                                             const int32_t* __restrict__ start, const float* __restrict__ dlogit) {
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= w.hdr[0]) return;
    const int32_t j = w.bucket[r];
    const int32_t L = count[j], s = start[j];
    int32_t rank = 0;
    for (int32_t i = 0; i < L; ++i) rank += (w.seg[s + i] < r);
    w.vals[s + rank] = dlogit[w.example[r]];
}

__global__ __launch_bounds__(kThreads) void wide_zero_untouched_kernel(const int32_t* __restrict__ count, int64_t H,
                                                                       float* __restrict__ kernel) {
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j < H && count[j] == 0) kernel[j] = 0.f;
}

__device__ __forceinline__ void ftrl_update(float g, float& var, float& accum, float& linear, float lr, float l1, float l2) {
    const float new_accum = accum + g * g;
    const float s_new = sqrtf(new_accum), s_old = sqrtf(accum);
    // sqrt(new_accum) - sqrt(accum), without the cancellation of the subtraction
    const float dsq = (s_new + s_old) > 0.f ? (g * g) / (s_new + s_old) : 0.f;
    linear += g - dsq / lr * var;
    const float quad = s_new / lr + 2.f * l2;
    const float sgn = linear > 0.f ? 1.f : (linear < 0.f ? -1.f : 0.f);
    var = fabsf(linear) > l1 ? (sgn * l1 - linear) / quad : 0.f;
    accum = new_accum;
}

// one thread per request; the thread of a bucket's first-counted request owns the bucket
__global__ __launch_bounds__(kThreads) void wide_apply_kernel(WideWs w, int32_t* __restrict__ count,
                                                              const int32_t* __restrict__ start, int mode,
                                                              float* __restrict__ kernel, float* __restrict__ kernel_grad,
                                                              float* __restrict__ accum, float* __restrict__ linear,
                                                              float* __restrict__ bias, float* __restrict__ bias_grad,
                                                              float* __restrict__ bias_accum, float* __restrict__ bias_linear,
                                                              float lr, float l1, float l2) {
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r == 0 && mode == RECALGO_WIDE_APPLY_FTRL) {
        w.hdr[1] = 0;
        if (bias) {
            float v = bias[0], a = bias_accum[0], l = bias_linear[0];
            ftrl_update(bias_grad[0], v, a, l, lr, l1, l2);
            bias[0] = v;
            bias_accum[0] = a;
            bias_linear[0] = l;
            bias_grad[0] = 0.f;
        }
    }
    if (r >= w.hdr[0] || w.slot[r] != 0) return;
    const int32_t j = w.bucket[r];
    const int32_t L = count[j], s = start[j];
    float g = 0.f;
    for (int32_t i = 0; i < L; ++i) g += w.vals[s + i];
    if (mode == RECALGO_WIDE_APPLY_GRAD) {
        kernel_grad[j] = g;
        return;
    }
    float v = kernel[j], a = accum[j], l = linear[j];
    ftrl_update(g, v, a, l, lr, l1, l2);
    kernel[j] = v;
    accum[j] = a;
    linear[j] = l;
    if (kernel_grad) kernel_grad[j] = 0.f;
    count[j] = 0;
}

__global__ __launch_bounds__(kThreads) void wide_reset_kernel(WideWs w, int32_t* __restrict__ count) {
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r == 0) w.hdr[1] = 0;
    if (r < w.hdr[0]) count[w.bucket[r]] = 0;
}


}  // namespace

RECALGO_EXPORT int64_t recalgo_wide_workspace_bytes(int capacity) {
    if (capacity < 0) return 0;
    return (16 + 5 * 4 * (int64_t)capacity + 15) / 16 * 16;
}

RECALGO_EXPORT int64_t recalgo_wide_state_workspace_bytes(int64_t hash_bucket_size) {
    if (hash_bucket_size < 1 || hash_bucket_size > RECALGO_WIDE_MAX_BUCKETS) return 0;
    return 2 * 4 * hash_bucket_size;
}

RECALGO_EXPORT int recalgo_wide_cross_fwd(const int64_t* user_ids, int64_t user_stride, const int64_t* tag_values,
                                          const int64_t* tag_offsets, int64_t tag_stride, int B, int capacity,
                                          int64_t hash_bucket_size, uint64_t hash_key, const float* kernel, const float* bias,
                                          void* ws, int32_t* state, float* wide_logit, recalgo_stream_t stream) {
    RECALGO_REQUIRE(user_ids && tag_values && kernel && ws && wide_logit);
    RECALGO_REQUIRE(B >= 1 && capacity >= 1 && user_stride >= 1 && aligned16(ws));
    RECALGO_REQUIRE(hash_bucket_size >= 1 && hash_bucket_size <= RECALGO_WIDE_MAX_BUCKETS);
    RECALGO_REQUIRE(tag_offsets || (tag_stride >= 1 && capacity >= B));
    hipLaunchKernelGGL(wide_fwd_kernel, dim3(cdiv(B, kThreads)), dim3(kThreads), 0, as_stream(stream), user_ids, user_stride,
                       tag_values, tag_offsets, tag_stride, B, capacity, (uint64_t)hash_bucket_size, hash_key, kernel, bias,
                       wide_ws(ws, capacity), state, wide_logit);
    RECALGO_RETURN_LAST();
}

// `state` = count[H], then start[H]
RECALGO_EXPORT int recalgo_wide_cross_plan(void* ws, int32_t* state, int capacity, int64_t hash_bucket_size,
                                           const float* dlogit, recalgo_stream_t stream) {
    RECALGO_REQUIRE(ws && state && dlogit && capacity >= 1 && aligned16(ws));
    RECALGO_REQUIRE(hash_bucket_size >= 1 && hash_bucket_size <= RECALGO_WIDE_MAX_BUCKETS);
    const WideWs w = wide_ws(ws, capacity);
    int32_t* start = state + hash_bucket_size;
    const dim3 grid(cdiv(capacity, kThreads)), block(kThreads);
    hipLaunchKernelGGL(wide_alloc_kernel, grid, block, 0, as_stream(stream), w, state, start);
    hipLaunchKernelGGL(wide_place_kernel, grid, block, 0, as_stream(stream), w, start);
    hipLaunchKernelGGL(wide_rank_kernel, grid, block, 0, as_stream(stream), w, state, start, dlogit);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_wide_cross_apply(void* ws, int32_t* state, int capacity, int64_t hash_bucket_size, int mode,
                                            float* kernel, float* kernel_grad, float* accum, float* linear, float* bias,
                                            float* bias_grad, float* bias_accum, float* bias_linear, float lr, float l1,
                                            float l2, int zero_untouched, recalgo_stream_t stream) {
    RECALGO_REQUIRE(ws && state && capacity >= 1 && aligned16(ws));
    RECALGO_REQUIRE(hash_bucket_size >= 1 && hash_bucket_size <= RECALGO_WIDE_MAX_BUCKETS);
    RECALGO_REQUIRE(mode == RECALGO_WIDE_APPLY_FTRL || mode == RECALGO_WIDE_APPLY_GRAD);
    if (mode == RECALGO_WIDE_APPLY_GRAD) {
        RECALGO_REQUIRE(kernel_grad && !zero_untouched);
    } else {
        RECALGO_REQUIRE(kernel && accum && linear && lr > 0.f && l1 >= 0.f && l2 >= 0.f);
        RECALGO_REQUIRE(!bias || (bias_grad && bias_accum && bias_linear));
    }
    if (zero_untouched)
        hipLaunchKernelGGL(wide_zero_untouched_kernel, dim3(cdiv(hash_bucket_size, kThreads)), dim3(kThreads), 0,
                           as_stream(stream), state, hash_bucket_size, kernel);
    hipLaunchKernelGGL(wide_apply_kernel, dim3(cdiv(capacity, kThreads)), dim3(kThreads), 0, as_stream(stream),
                       wide_ws(ws, capacity), state, state + hash_bucket_size, mode, kernel, kernel_grad, accum, linear, bias,
                       bias_grad, bias_accum, bias_linear, lr, l1, l2);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_wide_cross_reset(void* ws, int32_t* state, int capacity, recalgo_stream_t stream) {
    RECALGO_REQUIRE(ws && state && capacity >= 1 && aligned16(ws));
    hipLaunchKernelGGL(wide_reset_kernel, dim3(cdiv(capacity, kThreads)), dim3(kThreads), 0, as_stream(stream),
                       wide_ws(ws, capacity), state);
    RECALGO_RETURN_LAST();
}
