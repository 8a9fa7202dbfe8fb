// Ragged features in buffers of fixed capacity (include/recalgo_ragged.h): the two launches a captured step with bags needs
// beside the lookups it already has.  Both are small and memory-bound; what matters is that every launch has a grid sized from
// `capacity` alone (nothing read back) and that stores are whole, coalesced 16-byte pieces.
//   * ragged_pad_kernel: copy + -1 fill of an int64 buffer in one pass, two entries (16 bytes) per thread;
//   * bag_grad_rows_kernel: one thread per 16-byte piece (or per float) of rows[capacity, K].  The threads of an entry find its
//     bag by a binary search over offsets (they read the same addresses: one request per wave instruction) and count the
//     bag's valid values: where the Q threads of an entry are an aligned group of lanes (Q a power of two), each counts every
//     Q-th value and the group adds up by shuffles; otherwise each counts the whole bag (at most 50 values in the reference's
//     data).  The count is an integer either way: the same divisor, the same bits.
#include "common.h"
#include "../../include/recalgo_ragged.h"

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void ragged_pad_kernel(const int64_t* __restrict__ src, long long n,
                                                              int64_t* __restrict__ dst, long long capacity, int vec) {
    const long long i = 2 * ((long long)blockIdx.x * kThreads + threadIdx.x);
    if (i >= capacity) return;
    const long long a = i < n ? src[i] : -1ll;
    if (i + 1 < capacity) {
        const long long b = i + 1 < n ? src[i + 1] : -1ll;
        if (vec) {
            *reinterpret_cast<longlong2*>(dst + i) = make_longlong2(a, b);
        } else {
            dst[i] = a;
            dst[i + 1] = b;
        }
    } else {
        dst[i] = a;
    }
}

// the bag of entry j < nnz: #{ i in 1 .. B : offsets[i] <= j }, the number of bag ends at or before j
__device__ __forceinline__ int bag_of(const int64_t* __restrict__ offsets, int B, long long j) {
    int lo = 0, hi = B;                                   // offsets[1 + i] <= j for i < lo, > j for i >= hi
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (offsets[1 + mid] <= j) lo = mid + 1;
        else hi = mid;
    }
    return min(lo, B - 1);
}

// the valid values of the bag, as the float the division takes (an integer below 2^24 for any bag that fits a launch: exact)
// q, Q: this thread's place among the Q threads of the entry when they share the count (Q lanes, aligned: SPLIT), else 0, 1
template <bool SPLIT>
__device__ __forceinline__ float bag_count(const int64_t* __restrict__ values, const int64_t* __restrict__ offsets, int b, long long nnz,
                                           int q, int Q) {
    const long long lo = max(0ll, (long long)offsets[b]), hi = min(nnz, (long long)offsets[b + 1]);
    int cnt = 0;
    for (long long i = lo + (SPLIT ? q : 0); i < hi; i += SPLIT ? Q : 1) cnt += values[i] >= 0 ? 1 : 0;
    if (SPLIT) {                                          // (every lane of the group is here: they share j, hence `valid`)
        for (int o = Q >> 1; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    }
    return (float)max(cnt, 1);
}

// Q = pieces per row: K / 4 (VEC, float4 pieces) or K (floats)
template <bool VEC, bool SPLIT>
__global__ __launch_bounds__(kThreads) void bag_grad_rows_kernel(const int64_t* __restrict__ values, const int64_t* __restrict__ offsets,
                                                                 int B, long long capacity, const float* __restrict__ g, int g_stride,
                                                                 int g_col, int K, float* __restrict__ rows) {
    const int Q = VEC ? K >> 2 : K;
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= capacity * Q) return;
    const long long j = t / Q;
    const int q = (int)(t - j * Q);
    const long long nnz = B > 0 ? min((long long)offsets[B], capacity) : 0ll;
    const bool valid = j < nnz && values[j] >= 0;
    if (VEC) {
        float4 v = f4_zero();
        if (valid) {
            const int b = bag_of(offsets, B, j);
            const float c = bag_count<SPLIT>(values, offsets, b, nnz, q, Q);
            const float4 x = *reinterpret_cast<const float4*>(g + (size_t)b * g_stride + g_col + 4 * q);
            v = make_float4(__fdiv_rn(x.x, c), __fdiv_rn(x.y, c), __fdiv_rn(x.z, c), __fdiv_rn(x.w, c));
        }
        *reinterpret_cast<float4*>(rows + (size_t)j * K + 4 * q) = v;
    } else {
        float v = 0.f;
        if (valid) {
            const int b = bag_of(offsets, B, j);
            v = __fdiv_rn(g[(size_t)b * g_stride + g_col + q], bag_count<SPLIT>(values, offsets, b, nnz, q, Q));
        }
        rows[(size_t)j * K + q] = v;
    }
}

}  // namespace

RECALGO_EXPORT int recalgo_ragged_abi_version(void) { return RECALGO_RAGGED_ABI_VERSION; }

RECALGO_EXPORT int recalgo_ragged_pad(const int64_t* src, int64_t n, int64_t* dst, int64_t capacity, recalgo_stream_t stream) {
    RECALGO_REQUIRE(n >= 0 && n <= capacity && (dst || capacity == 0) && (src || n == 0));
    RECALGO_REQUIRE(aligned_to<8>(src) && aligned_to<8>(dst) && capacity < (1ll << 38));
    if (capacity == 0) return (int)hipSuccess;
    const long long pairs = (capacity + 1) / 2;
    hipLaunchKernelGGL(ragged_pad_kernel, dim3(cdiv(pairs, kThreads)), dim3(kThreads), 0, as_stream(stream), src, (long long)n, dst,
                       (long long)capacity, aligned_to<16>(dst) ? 1 : 0);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_bag_mean_grad_rows(const int64_t* values, const int64_t* offsets, int B, int64_t capacity, const float* g,
                                              int g_stride, int g_col, int K, float* rows, recalgo_stream_t stream) {
    RECALGO_REQUIRE(B >= 0 && capacity >= 0 && K >= 1 && g_col >= 0 && (int64_t)g_stride >= (int64_t)g_col + K && offsets);
    RECALGO_REQUIRE(capacity == 0 || (values && g && rows));
    RECALGO_REQUIRE(aligned_to<8>(values) && aligned_to<8>(offsets) && aligned_to<4>(g) && aligned_to<4>(rows));
    RECALGO_REQUIRE(capacity * (int64_t)K < (1ll << 38));
    if (capacity == 0) return (int)hipSuccess;
    const bool vec = K % 4 == 0 && g_stride % 4 == 0 && g_col % 4 == 0 && aligned16(g, rows);
    const int Q = vec ? K / 4 : K;
    // the Q threads of an entry are Q adjacent lanes of one wave, aligned to Q, exactly when Q is a power of two <= 64 (it then
    // divides the block and the wave): they share the count of the bag's valid values
    const bool split = Q > 1 && Q <= 64 && (Q & (Q - 1)) == 0;
    const dim3 grid(cdiv(capacity * Q, kThreads)), block(kThreads);
    auto* const kernel = vec ? (split ? bag_grad_rows_kernel<true, true> : bag_grad_rows_kernel<true, false>)
                             : (split ? bag_grad_rows_kernel<false, true> : bag_grad_rows_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, as_stream(stream), values, offsets, B, (long long)capacity, g, g_stride, g_col, K, rows);
    RECALGO_RETURN_LAST();
}
