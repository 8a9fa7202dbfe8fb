/* recalgo_ragged.h — tenth C-ABI header of librecalgo_hip.so: a ragged feature (values int64 [nnz], offsets int64 [B + 1]) held in
 * a buffer of FIXED capacity, so that a step with bags and histories has the same shapes on every batch and can be captured.
 *
 * The contract of a padded ragged feature (recalgorithm_amd/feature_column.py pad_ragged):
 *     values   int64 [capacity]; entries [offsets[B], capacity) are -1
 *     offsets  int64 [B + 1], unchanged; offsets[B] = nnz <= capacity
 * Every lookup reads `values` only through `offsets`, and the scatter treats an id < 0 as "no row", so the tail changes nothing.
 *
 * Self-contained (it repeats the stream typedef: an identical typedef twice is valid C11 and C++); the conventions are those of
 * recalgo.h: hipError_t as int, device pointers, asynchronous on `stream`, no hidden allocation, no host read-back
 * (hipGraph-capturable).
 */
#ifndef RECALGO_RAGGED_H_
#define RECALGO_RAGGED_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* recalgo_stream_t; /* hipStream_t */

/* ABI version of THIS header; include/recalgo_ragged.abi records the hash of the declarations each version stands for. */
#define RECALGO_RAGGED_ABI_VERSION 1
int recalgo_ragged_abi_version(void);

/* dst[0 : n] = src[0 : n];  dst[n : capacity] = -1 — ONE launch (a device-resident batch goes into a captured step's static
 * `values` buffer without a second fill launch).  src and dst do not overlap.
 * Refused with hipErrorInvalidValue before any launch: n < 0; n > capacity; a NULL dst with capacity > 0; a NULL src with n > 0; a
 * pointer that is not 8-byte aligned.  capacity == 0 launches nothing; n == 0 with src == NULL is valid (the whole buffer is -1). */
int recalgo_ragged_pad(const int64_t* src, int64_t n, int64_t* dst, int64_t capacity, recalgo_stream_t stream);

/* The gradient rows of a mean bag's entries, one launch: rows [capacity, K] fp32, contiguous, ALL of it written.
 *   entry j < min(offsets[B], capacity) with values[j] >= 0, lying in bag b (offsets[b] <= j < offsets[b + 1], found on the device):
 *       rows[j, :] = g[b * g_stride + g_col : .. + K] / (float)cnt_b     cnt_b = #{ i in bag b : values[i] >= 0 }
 *       an IEEE fp32 division of each element, as `g[bag] / cnt[bag]` of two fp32 tensors is
 *   every other row (an entry with values[j] < 0; the padding tail): zeros.
 * values: int64 [capacity] (a padded ragged feature, or capacity == nnz); offsets: int64 [B + 1], ascending from 0.  Neither
 * `values` nor `rows` is touched at or beyond `capacity`, whatever offsets holds.  The grid is sized from `capacity`: nothing is
 * read back.  K % 4 == 0 with 16-byte aligned g / rows and g_stride, g_col multiples of 4: one 16-byte store per thread;
 * otherwise one float per thread.
 * Refused with hipErrorInvalidValue before any launch: B < 0; capacity < 0; K < 1; g_col < 0; g_stride < g_col + K; a NULL offsets;
 * a NULL values, g or rows with capacity > 0; values / offsets not 8-byte or g / rows not 4-byte aligned; capacity * K >= 2^38.
 * capacity == 0 launches nothing. */
int recalgo_bag_mean_grad_rows(const int64_t* values, const int64_t* offsets, int B, int64_t capacity, const float* g, int g_stride,
                               int g_col, int K, float* rows, recalgo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECALGO_RAGGED_H_ */
