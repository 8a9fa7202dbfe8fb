// Shared device/host helpers for the recalgo HIP kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <mutex>

#include "../../include/recalgo.h"

#define RECALGO_EXPORT extern "C" __attribute__((visibility("default")))

// Every entry point returns hipError_t as int (0 == hipSuccess) and never throws.
#define RECALGO_RETURN_LAST()                  \
    do {                                       \
        hipError_t e__ = hipGetLastError();    \
        return (int)e__;                       \
    } while (0)

#define RECALGO_REQUIRE(cond)                          \
    do {                                               \
        if (!(cond)) return (int)hipErrorInvalidValue; \
    } while (0)

// Returns a failed hipError_t from the entry point (variadic: the expression may hold template argument lists).
#define RECALGO_CHECK(...)                          \
    do {                                            \
        hipError_t e__ = (__VA_ARGS__);             \
        if (e__ != hipSuccess) return (int)e__;     \
    } while (0)

static inline hipStream_t as_stream(recalgo_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

__host__ __device__ __forceinline__ int round4(int v) { return (v + 3) & ~3; }

// True when every pointer is N-byte aligned (N a power of two; a null pointer counts as aligned).
template <uintptr_t N, typename... P>
static inline bool aligned_to(const P*... p) {
    static_assert(N != 0 && (N & (N - 1)) == 0, "N is a power of two");
    return ((reinterpret_cast<uintptr_t>(p) | ... | (uintptr_t)0) & (N - 1)) == 0;
}
template <typename... P>
static inline bool aligned16(const P*... p) {
    return aligned_to<16>(p...);
}

// ---- dynamic LDS ----------------------------------------------------------
constexpr size_t kLdsDefault = 64 * 1024;   // dynamic LDS a kernel may claim without opting in
constexpr size_t kLdsMax = 160 * 1024;      // LDS of a gfx950 workgroup

// Launches Kernel with `lds` bytes of dynamic LDS: refuses more than kLdsMax, and above kLdsDefault raises the kernel's
// hipFuncAttributeMaxDynamicSharedMemorySize first.  The attribute belongs to (kernel, device), so each instantiation keeps
// the bytes it has been granted per device and calls the runtime only when a launch needs more (the lock keeps a smaller
// request of another host thread from lowering the attribute below that mark).  A failed launch is left for
// RECALGO_RETURN_LAST().
template <auto Kernel>
hipError_t grant_lds(size_t lds) {
    constexpr int kDevices = 64;
    static std::atomic<size_t> granted[kDevices] = {};
    static std::mutex grow;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= kDevices) return hipErrorInvalidDevice;
    if (lds <= granted[dev].load(std::memory_order_acquire)) return hipSuccess;
    std::lock_guard<std::mutex> lock(grow);
    if (lds <= granted[dev].load(std::memory_order_relaxed)) return hipSuccess;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) granted[dev].store(lds, std::memory_order_release);
    return e;
}
template <auto Kernel, typename... Args>
hipError_t launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    if (lds > kLdsMax) return hipErrorInvalidValue;
    if (lds > kLdsDefault) {
        const hipError_t e = grant_lds<Kernel>(lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
    return hipSuccess;
}

// ---- wave64 helpers -------------------------------------------------------
// Sum over all 64 lanes, result in every lane.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// Sum over aligned groups of W lanes (W = 4, 8, 16, 32), result in every lane of the group.
template <int W>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// LDS written by some lanes of a wave, read by others of the same wave
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Four consecutive floats: one 16-byte access when VEC (p 16-byte aligned), four scalar ones otherwise.
template <bool VEC>
__device__ __forceinline__ float4 ld4(const float* p) {
    if (VEC) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}
template <bool VEC>
__device__ __forceinline__ void st4(float* p, float4 v) {
    if (VEC) {
        *reinterpret_cast<float4*>(p) = v;
    } else {
        p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
    }
}

__device__ __forceinline__ float4 f4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 f4_add(float4 a, float4 b) {
    return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ float4 f4_scale(float4 a, float s) {
    return make_float4(a.x * s, a.y * s, a.z * s, a.w * s);
}
__device__ __forceinline__ float4 f4_fma(float4 a, float s, float4 c) {
    return make_float4(fmaf(a.x, s, c.x), fmaf(a.y, s, c.y), fmaf(a.z, s, c.z), fmaf(a.w, s, c.w));
}
__device__ __forceinline__ float f4_dot(float4 a, float4 b) {
    return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w)));
}

// Hardware fp32 atomic add (global_atomic_add_f32); build uses -munsafe-fp-atomics.
__device__ __forceinline__ void atomic_add_f32(float* p, float v) { unsafeAtomicAdd(p, v); }

// ---- deterministic column sum of partial rows ---------------------------------------------------
// out[c] = sum_{r < S} partials[r * n + c].  256 threads = 16 columns x 16 row groups: a thread adds
// rows rg, rg+16, ... in order, then the 16 groups are added in order (fixed summation order, and
// S/16 instead of S dependent loads per thread — the one-thread-per-column form of this loop cost
// 60-240 us for S = 256..1024 partial rows).  Columns [0, n0) go to out0, the rest to out1.
// The order is slab_sum.h's sum_tall: a caller's deferred form (a job of the step's sum launch) gives the same bits.
namespace {
__global__ __launch_bounds__(256) void colsum16_kernel(const float* __restrict__ partials, unsigned S, unsigned n,
                                                       float* __restrict__ out0, unsigned n0,
                                                       float* __restrict__ out1) {
    __shared__ float sh[16][17];
    const unsigned cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const unsigned c = blockIdx.x * 16 + cl;
    float acc = 0.f;
    if (c < n) {
        // independent loads, eight in flight per thread, added in row order (see dense_sum_slabs_kernel)
        const float* col = partials + c;
        unsigned r = rg;
        for (; r + 16 * 7 < S; r += 16 * 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = col[(size_t)(r + 16 * u) * n];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u];
        }
        for (; r < S; r += 16) acc += col[(size_t)r * n];
    }
    sh[rg][cl] = acc;
    __syncthreads();
    if (rg == 0 && c < n) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) t += sh[g][cl];
        if (c < n0) out0[c] = t;
        else out1[c - n0] = t;
    }
}
inline void launch_colsum16(const float* partials, unsigned S, unsigned n, float* out0, unsigned n0, float* out1,
                            hipStream_t st) {
    hipLaunchKernelGGL(colsum16_kernel, dim3((n + 15) / 16), dim3(256), 0, st, partials, S, n, out0, n0, out1);
}
}  // namespace
