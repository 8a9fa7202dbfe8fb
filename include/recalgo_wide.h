/* recalgo_wide.h — third C-ABI header of librecalgo_hip.so: the wide part of Wide&Deep
 * (algorithm/WideAndDeep/wide_and_deep.py:121-124,208-210,255-257): the crossed column of two int64 id features hashed on the
 * device, the one-unit dense layer over its (never materialised) multi-hot indicator, and tf.train.FtrlOptimizer applied
 * to the buckets a batch touched.  Self-contained (it repeats the stream typedef, as recalgo_cgc.h does); the conventions
 * are those of recalgo.h: hipError_t as int, device pointers, fp32, asynchronous on `stream`, no hidden allocation, no
 * float atomics (bit-reproducible, hipGraph-capturable).
 */
#ifndef RECALGO_WIDE_H_
#define RECALGO_WIDE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* recalgo_stream_t; /* hipStream_t */

/* ABI version of THIS header; include/recalgo_wide.abi records the hash of the declarations each version stands for. */
#define RECALGO_WIDE_ABI_VERSION 1
int recalgo_wide_abi_version(void);

#define RECALGO_WIDE_HASH_KEY 0xDECAFCAFFE      /* the default hash_key of tf.feature_column.crossed_column */
#define RECALGO_WIDE_MAX_BUCKETS 2147483647     /* hash_bucket_size: a bucket id is kept as int32 */
#define RECALGO_WIDE_APPLY_FTRL 0
#define RECALGO_WIDE_APPLY_GRAD 1

/* ------------------------------------------------------------------------------------------
 * The cross.  One REQUEST per (example b, entry t of example b's tag bag), numbered r = 0 .. n-1 in bag order:
 *   ShiftMix(v) = v ^ (v >> 47)
 *   Cat(a, b)   = kMul = 0xc6a4a7935bd1e995; r = a ^ kMul; r ^= ShiftMix(b * kMul) * kMul; r *= kMul;
 *                 r = ShiftMix(r) * kMul; ShiftMix(r)                       (uint64, wrapping: FingerprintCat64)
 *   bucket(r)   = Cat(Cat(hash_key, uint64(user_ids[b])), uint64(tag_values[t])) % hash_bucket_size
 * Ids are crossed as their int64 value: an out-of-vocabulary id of -1 is crossed as 0xFFFFFFFFFFFFFFFF.  An example with
 * an empty bag has no request.
 *
 *   user_ids     [B] int64, element b at user_ids[b * user_stride]
 *   tag_values   [capacity] int64; tag_offsets [B + 1] int64, bag b = tag_values[tag_offsets[b] .. tag_offsets[b + 1]).
 *                tag_offsets == NULL: one tag per example, tag_values[b * tag_stride] (capacity >= B).
 *                n = min(tag_offsets[B], capacity); bag bounds are clamped to [0, capacity]: nothing is read or written
 *                outside the buffers whatever the offsets hold.
 *   capacity     the FIXED request capacity the workspace is sized for (the length of tag_values): no buffer is sized by n
 *   ws           recalgo_wide_workspace_bytes(capacity) bytes, 16-byte aligned: the request count, bucket (int32) and
 *                example of every request, and the backward's plan.  Written by fwd, read by plan / apply / reset.
 *   state        recalgo_wide_state_workspace_bytes(hash_bucket_size) bytes, PERSISTENT and zero before the first call:
 *                per-bucket request count and segment start.  NULL (PREDICT / EVAL): nothing is counted.
 *                A forward with `state` must be followed by recalgo_wide_cross_apply(RECALGO_WIDE_APPLY_FTRL) or by
 *                recalgo_wide_cross_reset before the next one: both return the counts to zero.
 *   kernel       [hash_bucket_size] the (hash_bucket_size, 1) dense kernel; bias [1] or NULL
 *   wide_logit   [B]: bias + sum_{requests r of b} kernel[bucket(r)], added in request order (a bucket hit twice by one
 *                example counts twice: the indicator column sums its one-hots)
 * ------------------------------------------------------------------------------------------ */
int64_t recalgo_wide_workspace_bytes(int capacity);
int64_t recalgo_wide_state_workspace_bytes(int64_t hash_bucket_size);
int recalgo_wide_cross_fwd(const int64_t* user_ids, int64_t user_stride, const int64_t* tag_values,
                           const int64_t* tag_offsets, int64_t tag_stride, int B, int capacity, int64_t hash_bucket_size,
                           uint64_t hash_key, const float* kernel, const float* bias, void* ws, int32_t* state,
                           float* wide_logit, recalgo_stream_t stream);

/* The backward's plan over the requests of the last forward (three launches: segment allocation, placing, ranking):
 * the requests of a bucket get a segment of the workspace, and dlogit[example(r)] is stored in it at the RANK of r among
 * the bucket's request indices — so the per-bucket sum below runs in ascending request index whatever order the integer
 * atomics of counting and placing resolved in.  dlogit [B] = d loss / d wide_logit. */
int recalgo_wide_cross_plan(void* ws, int32_t* state, int capacity, int64_t hash_bucket_size, const float* dlogit,
                            recalgo_stream_t stream);

/* One thread per touched bucket j: g = sum of its segment (ascending request index), then
 *   RECALGO_WIDE_APPLY_GRAD: kernel_grad[j] = g; counts kept (an FTRL apply may follow)
 *   RECALGO_WIDE_APPLY_FTRL: TF's ApplyFtrl (lr_power = -0.5) in registers
 *       new_accum = accum + g * g
 *       linear   += g - (sqrt(new_accum) - sqrt(accum)) / lr * var       (the difference evaluated as
 *                                                                          g * g / (sqrt(new_accum) + sqrt(accum)))
 *       var       = |linear| > l1 ? (sign(linear) * l1 - linear) / (sqrt(new_accum) / lr + 2 * l2) : 0
 *       accum     = new_accum
 *     kernel_grad[j] = 0 when kernel_grad != NULL; the counts of `state` return to zero.
 *     bias != NULL: the same update for the one-element bias from bias_grad[0], which is then set to 0 (the dense Adam
 *     launch that sweeps the flat buffer afterwards is the identity on a slot with g = m = v = 0).
 *     zero_untouched != 0 (the FIRST FTRL step only): kernel[j] = 0 for every bucket without a request, in a launch of
 *     hash_bucket_size threads before the update — the dense update's result there (linear == 0 -> var = 0). */
int recalgo_wide_cross_apply(void* ws, int32_t* state, int capacity, int64_t hash_bucket_size, int mode, float* kernel,
                             float* kernel_grad, float* accum, float* linear, float* bias, float* bias_grad,
                             float* bias_accum, float* bias_linear, float lr, float l1, float l2, int zero_untouched,
                             recalgo_stream_t stream);

/* Return the counts of `state` to zero for the requests of the last forward (a step that never reached its apply). */
int recalgo_wide_cross_reset(void* ws, int32_t* state, int capacity, recalgo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECALGO_WIDE_H_ */
