/* recalgo_flen.h — C-ABI header of librecalgo_hip.so for FLEN's field-wise bi-interaction with Dicefactor (Chen et al., "FLEN:
 * Leveraging Field for Scalable CTR Prediction", arXiv 1911.04690), one kernel each way (csrc/flen.hip).
 * Self-contained (it repeats the stream typedef: an identical typedef twice is valid C11 and C++); the Dicefactor descriptor is
 * the recalgo_dropout_t of recalgo.h and is declared `const void*` here, with the type it points to.  The conventions are those
 * of recalgo.h: hipError_t as int, device pointers, fp32, asynchronous on `stream`, no hidden allocation, no host read-back, no
 * float atomics (bit-reproducible, hipGraph-capturable); descriptor arrays are HOST arrays read at launch time.
 */
#ifndef RECALGO_FLEN_H_
#define RECALGO_FLEN_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* recalgo_stream_t; /* hipStream_t */

/* ABI version of THIS header; include/recalgo_flen.abi records the hash of the declarations each version stands for. */
#define RECALGO_FLEN_ABI_VERSION 1
int recalgo_flen_abi_version(void);

#define RECALGO_FLEN_MIN_F 2
#define RECALGO_FLEN_MAX_F 64           /* fields */
#define RECALGO_FLEN_MIN_M 2
#define RECALGO_FLEN_MAX_M 8            /* field groups (M <= F, every group non-empty) */
#define RECALGO_FLEN_MIN_K 4
#define RECALGO_FLEN_MAX_K 64           /* embedding width (K % 4 == 0) */
#define RECALGO_FLEN_LANES 64           /* lanes of a workgroup: it serves floor(64 / (K / 4)) examples at a time */
#define RECALGO_FLEN_MAX_PARTIAL_ROWS 512   /* cap on the backward's partial rows, and on the workgroups of either launch */

/* ------------------------------------------------------------------------------------------
 * Per example.  x is [F, K], the field rows; group_of[f] in [0, M) maps the F fields onto M field groups; P = M (M - 1) / 2;
 * the pairs (i < j) of groups are in the order (0,1), (0,2), .., (0,M-1), (1,2), .. and p is the pair's index.
 *   e_m = sum_{f : group_of[f] = m} x_f            (ascending f)           [M, K]   the field-wise embeddings
 *   q_m = sum_{f : group_of[f] = m} x_f * x_f
 *   h   = bias + sum_p r_mf[p] c[p] * e_i * e_j + sum_m r_fm[m] c[P + m] * (e_m * e_m - q_m)                      [K]
 * (* is element-wise in the component k; e_m * e_m is rounded before q_m is subtracted, so a group of ONE field gives an FM
 * term of exactly 0.)  c [P + M, K] is the Dicefactor multiplier of each path component: 1 without Dicefactor (dice == NULL);
 * with it keep / (1 - rate), where the keep decision of flat element (b (P + M) + path) K + k is that of the recalgo_dropout_t
 * `dice` points to: its explicit keep_mask [B, P + M, K], or the hash of (seed, call, *step, element) of recalgo.h.
 *
 *   x, dx        [B, F K] contiguous            e, g_e   [B, M K]           h, g_h   [B, K]
 *   group_of     HOST int32 [F], read at launch time
 *   r_mf [P], r_fm [M], bias [K]                device
 *
 * backward (e and q are recomputed from x; the forward saves nothing else), with w_path = g_h * c[path]:
 *   t_m      = g_e[m] + sum_{pairs p containing m, partner j} r_mf[p] w_p * e_j
 *   dx_f     = t_m + 2 r_fm[m] w_{P+m} * (e_m - x_f)                      m = group_of[f]
 *   dr_mf[p] = sum_b sum_k w_p e_i e_j      dr_fm[m] = sum_b sum_k w_{P+m} (e_m^2 - q_m)      dbias = sum_b g_h
 * dx, dr_mf, dr_fm and dbias are OVERWRITTEN.  A group of K / 4 lanes serves an example, each lane four components, so a
 * workgroup of RECALGO_FLEN_LANES lanes serves T = floor(RECALGO_FLEN_LANES / (K / 4)) examples at a time; workgroup s of
 * R = recalgo_flen_bwd_partial_rows(B, F, M, K) = min(ceil(B / T), RECALGO_FLEN_MAX_PARTIAL_ROWS) takes the tiles s, s + R, ..
 * of T examples and leaves ONE partial row [dr_mf | dr_fm | dbias] of P + M + K floats in `workspace` (rows contiguous,
 * recalgo_flen_bwd_workspace_bytes = 4 R (P + M + K)).  The gradients are the fixed-order sums of the rows (the order of
 * recalgo_colsum_t, recalgo.h).  The forward runs min(ceil(B / T), RECALGO_FLEN_MAX_PARTIAL_ROWS) workgroups the same way.
 * An example's e, h and dx depend on that example alone: neither B nor its place in the batch changes a bit of them.
 *
 * Served (recalgo_flen_supported): 2 <= F <= 64; 2 <= M <= min(F, 8); K % 4 == 0 with 4 <= K <= 64; B >= 1; every group
 * non-empty.  An unsupported shape, B < 1, a group index outside [0, M), an empty group, a NULL pointer (dice excepted), x, dx,
 * e, g_e, h, g_h or an explicit keep mask not 16-byte aligned, r_mf, r_fm, bias, their gradients or the workspace not 4-byte
 * aligned, a dice rate outside (0, 1), or dice with B (P + M) K >= 2^32 returns hipErrorInvalidValue and launches nothing; the
 * queries return 0 for an unsupported shape or B < 1.
 * ------------------------------------------------------------------------------------------ */
int recalgo_flen_supported(int F, int M, int K);
int recalgo_flen_bwd_partial_rows(int B, int F, int M, int K);
int64_t recalgo_flen_bwd_workspace_bytes(int B, int F, int M, int K);
int recalgo_flen_fwd(const float* x, const int32_t* group_of, const float* r_mf, const float* r_fm, const float* bias,
                     const void* dice, int B, int F, int M, int K, float* e,
                     float* h, recalgo_stream_t stream);
int recalgo_flen_bwd(const float* g_e, const float* g_h, const float* x, const int32_t* group_of, const float* r_mf,
                     const float* r_fm, const void* dice, int B, int F, int M, int K, float* dx,
                     float* dr_mf, float* dr_fm, float* dbias, void* workspace, recalgo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECALGO_FLEN_H_ */
