/* recalgo_gauc.h — C-ABI header of librecalgo_hip.so for the per-group AUC of an evaluation (uAUC: the mean over users of each
 * user's own AUC; GAUC: the same, weighted by the user's rows): a per-batch append launch into a row log and a finish that groups
 * the log and counts pairs (recalgorithm_amd/estimator.py GroupAUCMetric, EvalAccumulator).  Self-contained (it repeats the
 * stream typedef: an identical typedef twice is valid C11 and C++); the conventions are those of recalgo.h and
 * recalgo_metrics.h: hipError_t as int, device pointers except the short HOST column table, fp32 inputs, int64 group ids,
 * asynchronous on `stream`, no hidden allocation, no host read-back (hipGraph-capturable).  Everything the kernels add up is an
 * integer, added with integer atomics: the counts depend neither on the order in which rows arrive nor on the order in which
 * they are grouped, so they are bit-reproducible.
 *
 * The metric, for rows (g, label, p) and G groups:
 *   a row with g < 0 or g >= G belongs to no group: it is counted in `skipped` and takes no further part;
 *   y = label > 0.5;  pos[u] = #{rows of group u with y},  neg[u] = #{rows of group u without};
 *   num2[u] = sum over (positive row i, negative row j) of group u of  2 [p_i > p_j] + [p_i == p_j],  both compared in fp32 on
 *   the values as stored (a NaN adds 0 against every partner, -0.0 ties with 0.0, +-inf order as usual);
 *   auc[u] = num2[u] / (2 pos[u] neg[u]) where pos[u] neg[u] > 0 — that division and the mean over groups are the host's.
 */
#ifndef RECALGO_GAUC_H_
#define RECALGO_GAUC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* recalgo_stream_t; /* hipStream_t */

/* ABI version of THIS header; include/recalgo_gauc.abi records the hash of the declarations each version stands for. */
#define RECALGO_GAUC_ABI_VERSION 1
int recalgo_gauc_abi_version(void);

#define RECALGO_GAUC_MAX_TASKS 8
#define RECALGO_GAUC_MAX_GROUPS 16777216 /* G: 1 .. 2^24 */
#define RECALGO_GAUC_MAX_ROWS 268435456  /* C, the capacity of the row log: 1 .. 2^28 (a position is an int32) */
#define RECALGO_GAUC_STATE_HEADER_WORDS 8
#define RECALGO_GAUC_RESULT_HEADER_WORDS 3

/* One task of the batch.  labels and predictions: fp32, element i at [i * step] (label_step, prediction_step: the element stride
 * of each, >= 1; column i of a [B, T] matrix has T). */
typedef struct {
    const float* labels;
    const float* predictions;
    int label_step, prediction_step;
} recalgo_gauc_column_t;

/* ------------------------------------------------------------------------------------------
 * Buffers, all caller-owned and 8-byte aligned.  Cp = C rounded up to a multiple of 4, Gp = G rounded up to a multiple of 256.
 *
 * state      recalgo_gauc_state_bytes(G, T, C) bytes; the caller zeroes the header (the first 64 bytes) before the first batch.
 *   header, int64 words:  0 cursor (rows appended so far, dropped ones included)   1 dropped (rows that found no room)
 *                         2 the arrival ticket of an append launch (zero between launches)   3 .. 7 reserved, zero
 *   the row log behind it:  int32 group[Cp]        the group of position k, -1 for a row that belongs to no group
 *                           float prediction[T][Cp]
 *                           uint8 labels[Cp]       bit t: label of task t > 0.5
 *   64 + Cp (5 + 4 T) bytes, rounded up to a multiple of 8.
 *
 * result     (3 + 3 T G) int64:  skipped, dropped, rows | num2 [T][G] | pos [T][G] | neg [T][G]
 *            rows = min(cursor, C), the rows in the log, the skipped ones among them: ONE device-to-host copy serves the host.
 *
 * workspace  recalgo_gauc_workspace_bytes(G, T, C) bytes, scratch of the finish, nothing to initialise:
 *            uint32 count[Gp], first[Gp], fill[Gp], tile_sum[Gp / 256 rounded up to 256, and 256 more], then the log once more
 *            in group order (int32 group[Cp], float prediction[T][Cp], uint8 labels[Cp]); rounded up to a multiple of 8.
 *
 * Both size queries are host-side and return 0 for a shape the launches refuse.
 *
 * recalgo_gauc_append — one launch per batch of n rows.  groups: int64, row i at [i * group_step] (a column of a packed
 * [B, F] id matrix has F).  columns: a HOST table of T entries.  Row i takes log position cursor + i and the cursor
 * then advances by n, whatever the rows hold (a row without a group is logged as such), so positions never depend on the
 * data.  A row whose position is >= C is not written and `dropped` grows by one.  The cursor lives on the device: every
 * workgroup reads it, the last one to finish advances it, so a captured launch appends behind its previous replay.
 *
 * recalgo_gauc_finish — once per evaluation, several launches: rows per group, an exclusive scan over the groups, the rows
 * placed by group (the order inside a group is free), the pair counts per task, `result` filled (all of it: the caller need
 * not zero it).  It reads the log and leaves it, and the state header, unchanged: appending more rows and finishing again
 * gives the counts over all rows so far.
 *
 * Refused with hipErrorInvalidValue before any launch: n < 1; T outside 1 .. 8; G outside 1 .. RECALGO_GAUC_MAX_GROUPS; C
 * outside 1 .. RECALGO_GAUC_MAX_ROWS; a NULL groups, columns, state, result, workspace, labels or predictions; a step < 1;
 * a float pointer that is not 4-byte aligned; groups, state, result or workspace not 8-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int64_t recalgo_gauc_state_bytes(int G, int T, int C);
int64_t recalgo_gauc_workspace_bytes(int G, int T, int C);
int recalgo_gauc_append(const int64_t* groups, int group_step, const recalgo_gauc_column_t* columns, int T, int n, int G, int C,
                        void* state, recalgo_stream_t stream);
int recalgo_gauc_finish(const void* state, int G, int T, int C, int64_t* result, void* workspace, recalgo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECALGO_GAUC_H_ */
