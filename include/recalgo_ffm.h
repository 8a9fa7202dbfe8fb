/* recalgo_ffm.h — C-ABI header of librecalgo_hip.so for FFM's field-aware second-order term (algorithm/FFM/ffm.py:146-160) as
 * one kernel each way that fetches its rows itself, and the de-duplication of a bag field on the device (csrc/ffm.hip).
 * Self-contained (it repeats the stream typedef: an identical typedef twice is valid C11 and C++); the deferred-Adam descriptor
 * is that of recalgo.h and is declared `const void*` here, with the type it points to.  The conventions are those of
 * recalgo.h: hipError_t as int, device pointers, fp32, asynchronous on `stream`, no hidden allocation, no host read-back, no
 * float atomics (bit-reproducible, hipGraph-capturable); descriptor arrays are HOST arrays read at launch time.
 */
#ifndef RECALGO_FFM_H_
#define RECALGO_FFM_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* recalgo_stream_t; /* hipStream_t */

/* ABI version of THIS header; include/recalgo_ffm.abi records the hash of the declarations each version stands for. */
#define RECALGO_FFM_ABI_VERSION 1
int recalgo_ffm_abi_version(void);

#define RECALGO_FFM_MIN_F 2         /* fields */
#define RECALGO_FFM_MAX_F 32
#define RECALGO_FFM_MIN_K 4         /* embedding width, K % 4 == 0: a row is K / 4 pieces of 16 bytes */
#define RECALGO_FFM_MAX_K 64
#define RECALGO_FFM_MAX_BAGS 4      /* multi-valued (bag) fields */

/* 1 when (F fields, width K, n_bags of the fields multi-valued) is served: RECALGO_FFM_MIN_F <= F <= RECALGO_FFM_MAX_F,
 * RECALGO_FFM_MIN_K <= K <= RECALGO_FFM_MAX_K with K % 4 == 0, 0 <= n_bags <= min(F, RECALGO_FFM_MAX_BAGS); else 0. */
int recalgo_ffm_supported(int F, int K, int n_bags);

/* ------------------------------------------------------------------------------------------
 * The distinct ids of every bag (utils.py:49-64 `to_sparse_tensor`), one launch, shapes fixed by (B, n) alone.
 *   values [n] int64, offsets [B + 1] int64 (offsets[0] == 0, non-decreasing; entries from offsets[B] on belong to no bag: the -1
 *   tail of a Ragged padded to a capacity of n)
 *   out_values [n]  entry j < min(offsets[B], n) keeps its id when the id is >= 0 and no EARLIER entry of its bag holds the same
 *                   id; every other entry (a repeated id, an id < 0, the tail) becomes -1.  out_values may not alias values.
 *   valid [B] int32     the bag's entries with an id >= 0, a repeated id counted every time
 *   distinct [B] int32  the bag's kept entries
 * The bag of an entry is found on the device (a binary search over offsets); any bag length is served (an entry compares with
 * the earlier entries of its bag one by one).  Refused (hipErrorInvalidValue, nothing launched): B <= 0, n < 0, B + n >= 2^31, a
 * NULL offsets / valid / distinct, a NULL values / out_values with n > 0, out_values == values with n > 0, int64 arrays not
 * 8-byte and int32 arrays not 4-byte aligned. */
int recalgo_ffm_bag_distinct(const int64_t* values, const int64_t* offsets, int B, int64_t n, int64_t* out_values, int32_t* valid,
                             int32_t* distinct, recalgo_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * out[b] = sum over the pairs i < j of < v_i[j - 1], v_j[i] >                                  (ffm.py:146-160)
 * Field i owns F - 1 sub-tables of `vocab` rows each, one after the other in the arena from row `row_base`: v_i[s] is arena row
 * row_base + s * vocab + id (int64 arithmetic), and
 *   a single-valued field (bag < 0)  reads its id of example b at ids[b * n_single + column], column = the number of single-valued
 *                                    fields before it; v_i[s] = 0 for an id < 0 (OOV)
 *   a bag field (bag = its index in `bags`)  v_i[s] = the mean of those rows over the entries offsets[b] <= e < offsets[b + 1]
 *                                    (clipped to [0, capacity)) with values[e] >= 0, summed in bag order and divided by
 *                                    distinct[b]; 0 when distinct[b] <= 0.  values / distinct are those that
 *                                    recalgo_ffm_bag_distinct left.
 * Every field of a call names a different bag, and every bag is named.  A wave serves an example; rows move as 16-byte pieces.
 */
typedef struct {
    int64_t row_base;               /* arena row of row 0 of sub-table 0 */
    int64_t vocab;                  /* rows per sub-table, >= 1 */
    int bag;                        /* < 0: single-valued; else index into `bags` */
} recalgo_ffm_field_t;
typedef struct {
    const int64_t* values;          /* [capacity], de-duplicated: an entry < 0 is no row */
    const int64_t* offsets;         /* [B + 1] */
    const int32_t* distinct;        /* [B] */
    int64_t capacity;               /* entries of values (and rows of d_rows), >= 0, < 2^31 */
    float* d_rows;                  /* backward only: [capacity, (F - 1) K], 16-byte aligned */
} recalgo_ffm_bag_t;

/*   ids      [B, n_single] int64 (NULL when every field is a bag)       fields  HOST [F]        bags  HOST [n_bags] (NULL: none)
 *   arena    [rows, K] fp32, 16-byte aligned                             out     [B]
 *   deferred const recalgo_deferred_adam_t* of recalgo.h, or NULL; step_dev, step_offset: as the *_fwd_deferred lookups of
 *            recalgo.h — a row whose state lags is read as of step step_dev[0] + step_offset, replayed in registers, nothing
 *            written back (PREDICT / EVAL between training steps).  NULL (or no last_step, or step_dev NULL): a plain read.
 * Writes nothing but out.
 *
 * backward: the gradient rows of the requests, fetched again from the arena (plain reads: the rows of a training lookup were
 * caught up before its forward and do not change before the optimizer applies the step); nothing is saved by the forward.
 *   g         [B]: d loss / d out
 *   d_single  [B, n_single (F - 1) K], 16-byte aligned (NULL when every field is a bag): request (b, column a', sub-table s) of
 *             single-valued field a = g[b] * v_partner, the partner of (a, s) being (s + 1, a) when s >= a, else (s, a - 1)
 *   bags[k].d_rows [capacity, (F - 1) K]: entry e of example b's bag with values[e] >= 0 gets (g[b] / distinct[b]) * v_partner
 *             at sub-table s; every other entry of the buffer gets zeros.
 * Every element of d_single and of every d_rows is written exactly once.
 *
 * Refused (hipErrorInvalidValue, nothing launched): a shape recalgo_ffm_supported refuses, B <= 0, B * n_single * (F - 1) * K / 4
 * >= 2^31, a NULL fields / arena / out (g), a NULL ids / d_single with a single-valued field, NULL bags with n_bags > 0, a field
 * with vocab < 1 or row_base < 0 or a bag index outside [0, n_bags) or one already taken, a bag with a NULL offsets / distinct,
 * capacity outside [0, 2^31), a NULL values (d_rows) with capacity > 0, int64 arrays not 8-byte, int32 / float arrays not
 * 4-byte, arena / d_single / d_rows not 16-byte aligned. */
int recalgo_ffm_fwd(const int64_t* ids, const recalgo_ffm_field_t* fields, const recalgo_ffm_bag_t* bags, int n_bags,
                    const float* arena, int B, int F, int K, float* out, const void* deferred, const int64_t* step_dev,
                    int step_offset, recalgo_stream_t stream);
int recalgo_ffm_bwd(const float* g, const int64_t* ids, const recalgo_ffm_field_t* fields, const recalgo_ffm_bag_t* bags, int n_bags,
                    const float* arena, int B, int F, int K, float* d_single, recalgo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECALGO_FFM_H_ */
