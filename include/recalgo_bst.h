/* recalgo_bst.h — fourth C-ABI header of librecalgo_hip.so: the transformer block of BST
 * (algorithm/BST/transformer_layer.py:6-81), two kernels each way.  Self-contained (it repeats the stream typedef: an
 * identical typedef twice is valid C11 and C++); the conventions are those of recalgo.h: hipError_t as int, device
 * pointers, fp32, asynchronous on `stream`, no hidden allocation, no float atomics (bit-reproducible, hipGraph-capturable).
 */
#ifndef RECALGO_BST_H_
#define RECALGO_BST_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* recalgo_stream_t; /* hipStream_t */

/* ABI version of THIS header; include/recalgo_bst.abi records the hash of the declarations each version stands for. */
#define RECALGO_BST_ABI_VERSION 1
int recalgo_bst_abi_version(void);

#define RECALGO_BST_MAX_T 64    /* rows of one example: the target and its history */
#define RECALGO_BST_MAX_D 16    /* embedding width d = d_k = d_model (d % 4 == 0) */
#define RECALGO_BST_MAX_HEADS 4 /* H */

/* ------------------------------------------------------------------------------------------
 * One block, per example (x [T, d]: the target row, the history rows, zero rows of padding; L = keys_length clamped to
 * [0, T]):
 *   Xp   = x + pos[0:T]
 *   Q_h  = Xp w_q[h]     K_h = Xp w_k[h]     V_h = x w_v[h]                 (V from x, NOT from Xp)
 *   S_h  = Q_h K_h^T / sqrtf(d)            (an fp32 DIVISION), then  S_h[i][:] += -4294967296.0f  for every QUERY row
 *                                           i >= L, as a literal fp32 add: it absorbs every |s| < 128, so such a row's
 *                                           softmax is uniform 1/T; its gradient is the identity
 *   P_h  = softmax(S_h) over the T keys (padded ones included; max-subtracted)
 *   n1   = LayerNorm(concat_h(P_h V_h) w_o + Xp)
 *   out  = LayerNorm(leakyrelu(n1 W + b) + n1),   leakyrelu(v) = 0.505 v + 0.495 |v|
 *   pool = sum_t out[t]  (mean_pool: / T), all T rows
 * LayerNorm: moments per example over the whole [T, d] block, mean and var = mean((v - mean)^2) accumulated in double,
 * rstd = 1 / sqrt(var + 1e-12), result (v - mean) * rstd * gamma[j] + beta[j].  A constant [T, d] block is singular.
 *
 *   x, n1, out, g_*  [B, T, d] contiguous        pos  [>= T, d] (rows 0..T-1 are read)     keys_length  int32 [B]
 *   w_q, w_k, w_v    [H, d, d]                   w_o  [H * d, d]                             gamma, beta  [d]
 *   ffn_w [d, d]     ffn_b [d]                   pool, g_pool [B, d]
 *   stats            [B, 2] (mean, rstd) as fp32, or NULL: for the caller; the backward entries recompute both in double
 *
 * Backward entries recompute everything from the forward's INPUTS (no [B, H, T, T] tensor exists in memory).
 *   attn_bwd: dx [B, T, d] = Q/K path + V path + residual path; dpos [T, d] (the sum over the batch of the Xp gradient);
 *             dw_q, dw_k, dw_v, dw_o, dgamma, dbeta shaped like their parameters.
 *   ffn_bwd:  g_out and / or g_pool (one may be NULL); dn1 [B, T, d]; dw, db, dgamma, dbeta.
 * Parameter gradients, two passes: workgroup r of the backward grid (recalgo_bst_*_bwd_partial_rows(B) workgroups) adds
 * the examples r, r + rows, r + 2 rows, .. in that order into row r of `workspace`
 * ([rows][T d + 4 H d d + 2 d] resp. [rows][d d + 3 d] floats, recalgo_bst_*_bwd_workspace_bytes); the same entry then
 * sums the rows column-wise in row order.  Two runs on the same inputs are bit-equal; a permutation of the examples
 * changes which partial row an example joins, so parameter gradients are equal under it only up to fp32 summation
 * order (dx / dn1 rows are independent of it).
 *
 * Served (recalgo_bst_supported; anything else, B < 1, a NULL pointer other than the optional ones, or a pointer that is
 * not 4-byte aligned returns hipErrorInvalidValue and launches nothing): 1 <= T <= 64, d in {4, 8, 12, 16}, 1 <= H <= 4.
 * ------------------------------------------------------------------------------------------ */
int recalgo_bst_supported(int T, int d, int H);
int recalgo_bst_attn_bwd_partial_rows(int B);
int64_t recalgo_bst_attn_bwd_workspace_bytes(int B, int T, int d, int H);
int recalgo_bst_ffn_bwd_partial_rows(int B);
int64_t recalgo_bst_ffn_bwd_workspace_bytes(int B, int d);
int recalgo_bst_attn_fwd(const float* x, const float* pos, const int32_t* keys_length, const float* w_q, const float* w_k,
                         const float* w_v, const float* w_o, const float* gamma, const float* beta, int B, int T, int d,
                         int H, float* n1, float* stats, recalgo_stream_t stream);
int recalgo_bst_attn_bwd(const float* x, const float* pos, const int32_t* keys_length, const float* w_q, const float* w_k,
                         const float* w_v, const float* w_o, const float* gamma, const float* g_n1, int B, int T, int d,
                         int H, float* dx, float* dpos, float* dw_q, float* dw_k, float* dw_v, float* dw_o, float* dgamma,
                         float* dbeta, float* workspace, recalgo_stream_t stream);
int recalgo_bst_ffn_fwd(const float* n1, const float* ffn_w, const float* ffn_b, const float* gamma, const float* beta, int B,
                        int T, int d, int mean_pool, float* out, float* pool, float* stats, recalgo_stream_t stream);
int recalgo_bst_ffn_bwd(const float* n1, const float* ffn_w, const float* ffn_b, const float* gamma, const float* g_out,
                        const float* g_pool, int B, int T, int d, int mean_pool, float* dn1, float* dw, float* db,
                        float* dgamma, float* dbeta, float* workspace, recalgo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECALGO_BST_H_ */
