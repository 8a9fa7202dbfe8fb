/* recalgo_metrics.h — eighth C-ABI header of librecalgo_hip.so: the streaming evaluation metrics of an EVAL batch
 * (tf.metrics.auc with its threshold array, tf.metrics.accuracy; recalgorithm_amd/estimator.py EvalAccumulator) and the loss
 * accumulator, as ONE launch per batch.  Self-contained (it repeats the stream typedef: an identical typedef twice is valid C11
 * and C++); the conventions are those of recalgo.h: hipError_t as int, device pointers except the short HOST slot table, fp32
 * inputs, asynchronous on `stream`, no hidden allocation, no host read-back (hipGraph-capturable).  Everything the kernel adds
 * is an integer, added with integer atomics: the counts do not depend on the order of the additions, so they are bit-reproducible.
 */
#ifndef RECALGO_METRICS_H_
#define RECALGO_METRICS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* recalgo_stream_t; /* hipStream_t */

/* ABI version of THIS header; include/recalgo_metrics.abi records the hash of the declarations each version stands for. */
#define RECALGO_METRICS_ABI_VERSION 1
int recalgo_metrics_abi_version(void);

#define RECALGO_METRICS_MAX_SLOTS 16
#define RECALGO_METRICS_MAX_THRESHOLDS 1024 /* N of an AUC slot, >= 2 */
#define RECALGO_METRICS_AUC 0
#define RECALGO_METRICS_ACCURACY 1

/* One metric of the batch.  labels and predictions: fp32, element i at [i * stride] (stride in elements, >= 1: column i of a
 * [B, T] matrix has stride T).  thresholds: N fp32 values in ascending order (AUC only; not read for ACCURACY). */
typedef struct {
    const float* labels;
    const float* predictions;
    const float* thresholds;
    int kind; /* RECALGO_METRICS_AUC | RECALGO_METRICS_ACCURACY */
    int num_thresholds;
    int label_stride, prediction_stride;
} recalgo_metrics_slot_t;

/* ------------------------------------------------------------------------------------------
 * The state buffer, caller-owned, 8-byte aligned, zeroed by the caller before the first batch; 64-bit words:
 *   word 0                  double  loss_sum
 *   word 1                  int64   batches
 *   then, slot after slot in table order,
 *     AUC(N):     2 (N + 1) int64   hist[y][bin], y = 0 | 1 major, bin = 0 .. N
 *     ACCURACY:   2         int64   correct, total
 * recalgo_metrics_state_bytes: the size of that buffer for a slot table (it reads kind and num_thresholds only); 0 for a table
 * recalgo_metrics_update would refuse for its kinds or sizes.  A host-side query.
 *
 * recalgo_metrics_update, for the n rows of one batch:
 *   AUC        y = labels[i] > 0.5;  bin = #{ j : predictions[i] > thresholds[j] }, compared in fp32 against the array as passed
 *              (a NaN prediction compares false everywhere: bin 0);  hist[y][bin] += 1
 *              (so tp[j] = sum over bin > j of hist[1][bin], fp[j] likewise of hist[0]: the host does that once, at the end)
 *   ACCURACY   correct += #{ i : labels[i] == predictions[i] };  total += n
 *   loss       (device pointer to the batch's fp32 scalar loss; NULL: the two words are left alone)
 *              loss_sum += (double)*loss;  batches += 1 — by one thread: successive launches on one stream add in launch order,
 *              the same sequence of double additions as a host loop over the batches.
 *
 * Refused with hipErrorInvalidValue before any launch: n < 1; n_slots outside 1 .. 16; a NULL slots, state, labels or
 * predictions, or a NULL thresholds of an AUC slot; a kind other than the two; N outside 2 .. 1024; a stride < 1; a float
 * pointer (loss included) that is not 4-byte aligned; a state that is not 8-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int64_t recalgo_metrics_state_bytes(const recalgo_metrics_slot_t* slots, int n_slots);
int recalgo_metrics_update(const recalgo_metrics_slot_t* slots, int n_slots, const float* loss, int n, void* state,
                           recalgo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECALGO_METRICS_H_ */
