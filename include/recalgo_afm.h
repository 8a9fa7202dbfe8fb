/* recalgo_afm.h — C-ABI header of librecalgo_hip.so for AFM's attention network (algorithm/AFM/afm.py:162-188), one kernel
 * each way.  Self-contained (it repeats the stream typedef: an identical typedef twice is valid C11 and C++); the conventions
 * are those of recalgo.h: hipError_t as int, device pointers, fp32, asynchronous on `stream`, no hidden allocation, no float
 * atomics (bit-reproducible, hipGraph-capturable).
 */
#ifndef RECALGO_AFM_H_
#define RECALGO_AFM_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* recalgo_stream_t; /* hipStream_t */

/* ABI version of THIS header; include/recalgo_afm.abi records the hash of the declarations each version stands for. */
#define RECALGO_AFM_ABI_VERSION 1
int recalgo_afm_abi_version(void);

#define RECALGO_AFM_MAX_F 64        /* fields: P = F (F - 1) / 2 <= 2016 pairs */
#define RECALGO_AFM_MAX_K 32        /* embedding width (K % 4 == 0, K >= 4) */
#define RECALGO_AFM_MAX_T 256       /* attention factor t (t % 16 == 0, t >= 16) */
#define RECALGO_AFM_MAX_PARTIAL_ROWS 1024

/* ------------------------------------------------------------------------------------------
 * With e_0 .. e_{F-1} the F rows [K] of one example of `fields` and the pairs p = (i, j), i < j, in row-major order over the
 * strict upper triangle (P = F (F - 1) / 2 of them):
 *   pair_p = e_i * e_j                                        (Hadamard)
 *   s_p    = sum_c relu(pair_p . w[:, c] + b[c]) * h[c]       w [K, t] row-major, b [t], h [t]
 *   a      = softmax(s) over the P pairs (shifted by max s)
 *   out    = sum_p a_p pair_p                                 [K]
 * Every dot product over K is a k-ordered fp32 fmaf chain (v_mfma_f32_16x16x4_f32); a score is summed over t in double.
 *
 *   fields, d_fields   [B, F K] contiguous
 *   out, g             [B, K]
 *   scores             [B, P]: the s_p (forward: written when not NULL — PREDICT / EVAL pass NULL; backward: read)
 *
 * backward (relu(pair w + b) is recomputed, the softmax is taken from `scores`):
 *   da_p = g . pair_p      ds_p = a_p (da_p - sum_q a_q da_q)      dz_p = ds_p h * [pair_p w + b > 0]      [t]
 *   dpair_p = dz_p w^T + a_p g
 *   d_fields[i] = sum over the partners j of i, in field order, of dpair_(i,j) * e_j
 *   dw = sum pair_p^T dz_p [K, t],  db = sum dz_p [t],  dh = sum ds_p relu(pair_p w + b) [t]   over all pairs and examples
 * d_fields, dw, db and dh are OVERWRITTEN.  A workgroup serves `waves` examples at a time (4, or 2 or 1 where the LDS of a
 * workgroup does not hold four examples' state) and leaves ONE partial row [dw | db | dh] of K t + 2 t floats in `workspace`:
 * recalgo_afm_bwd_partial_rows(B, F, K, t) = min(ceil(B / waves), RECALGO_AFM_MAX_PARTIAL_ROWS) rows, contiguous,
 * recalgo_afm_bwd_workspace_bytes = rows * (K t + 2 t) * 4.  dw, db, dh are the fixed-order sums of the rows (the order of
 * recalgo_colsum_t, recalgo.h).  A row's out, scores and d_fields depend on that row alone: neither B nor a row's place in the
 * batch changes a bit of them.
 *
 * Served (recalgo_afm_supported): 2 <= F <= 64, 4 <= K <= 32 with K % 4 == 0, 16 <= t <= 256 with t % 16 == 0; B >= 1.  An
 * unsupported shape, B < 1, a NULL pointer (`scores` excepted in the forward) or a pointer that is not 4-byte aligned returns
 * hipErrorInvalidValue and launches nothing; the two queries return 0 for an unsupported shape or B < 1.
 * ------------------------------------------------------------------------------------------ */
int recalgo_afm_supported(int F, int K, int t);
int recalgo_afm_bwd_partial_rows(int B, int F, int K, int t);
int64_t recalgo_afm_bwd_workspace_bytes(int B, int F, int K, int t);
int recalgo_afm_attention_fwd(const float* fields, const float* w, const float* b, const float* h, int B, int F, int K, int t,
                              float* out, float* scores, recalgo_stream_t stream);
int recalgo_afm_attention_bwd(const float* g, const float* fields, const float* w, const float* b, const float* h,
                              const float* scores, int B, int F, int K, int t, float* d_fields, float* dw, float* db, float* dh,
                              void* workspace, recalgo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECALGO_AFM_H_ */
