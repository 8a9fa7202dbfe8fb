// Byte-exact copy of one device span by a grid of threads: the body of copy_bytes_kernel (tail.hip) and of the copy workgroups of
// sparse_prepare_kernel (sparse.hip), stated once.  dst and src share their 16-byte phase (copy_span_split): a vector body of
// n16 16-byte pieces between a head and a tail of single bytes.
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace recalgo_copy {

// thread t of T (T a multiple of the workgroup size, every thread of the grid calls): 16 bytes per thread and pass, four loads in
// flight per thread for large spans; the head is moved by threads [0, head), the tail by threads [0, 16)
__device__ __forceinline__ void copy_span(unsigned char* __restrict__ dst, const unsigned char* __restrict__ src, size_t head, size_t n16,
                                          size_t nbytes, size_t t, size_t T) {
    const uint4* s16 = reinterpret_cast<const uint4*>(src + head);
    uint4* d16 = reinterpret_cast<uint4*>(dst + head);
    size_t i = t;
    for (; i + 3 * T < n16; i += 4 * T) {
        const uint4 a = s16[i], b = s16[i + T], c = s16[i + 2 * T], d = s16[i + 3 * T];
        d16[i] = a; d16[i + T] = b; d16[i + 2 * T] = c; d16[i + 3 * T] = d;
    }
    for (; i < n16; i += T) d16[i] = s16[i];
    if (t < head) dst[t] = src[t];
    const size_t tail0 = head + n16 * 16;
    if (tail0 + t < nbytes && t < 16) dst[tail0 + t] = src[tail0 + t];
}

// host: head bytes and 16-byte pieces of a span of nbytes > 0; false when dst and src differ in their 16-byte phase
inline bool copy_span_split(const void* dst, const void* src, size_t nbytes, size_t* head, size_t* n16) {
    const uintptr_t d = reinterpret_cast<uintptr_t>(dst), s = reinterpret_cast<uintptr_t>(src);
    if ((d & 15) != (s & 15)) return false;
    size_t h = (16 - (d & 15)) & 15;
    if (h > nbytes) h = nbytes;
    *head = h;
    *n16 = (nbytes - h) / 16;
    return true;
}

// workgroups of 256 threads that copy_span is launched with: one 16-byte piece per thread up to 2048 workgroups
inline unsigned copy_span_blocks(size_t n16) {
    const size_t want = (n16 + 255) / 256;
    return (unsigned)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
}

}  // namespace recalgo_copy
