/* recalgo_autoint.h — C-ABI header of librecalgo_hip.so for AutoInt's interacting layer (Song et al., CIKM 2019, arXiv
 * 1810.11921, eqs. 5-8): multi-head self-attention over the F fields of one example, one kernel each way.  Self-contained (it
 * repeats the stream typedef: an identical typedef twice is valid C11 and C++); the conventions are those of recalgo.h:
 * hipError_t as int, device pointers, fp32, asynchronous on `stream`, no hidden allocation, no float atomics (bit-reproducible,
 * hipGraph-capturable).
 */
#ifndef RECALGO_AUTOINT_H_
#define RECALGO_AUTOINT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* recalgo_stream_t; /* hipStream_t */

/* ABI version of THIS header; include/recalgo_autoint.abi records the hash of the declarations each version stands for. */
#define RECALGO_AUTOINT_ABI_VERSION 1
int recalgo_autoint_abi_version(void);

#define RECALGO_AUTOINT_MIN_F 2
#define RECALGO_AUTOINT_MAX_F 64        /* fields */
#define RECALGO_AUTOINT_MIN_D 4
#define RECALGO_AUTOINT_MAX_D 64        /* input width of a layer (D % 4 == 0) */
#define RECALGO_AUTOINT_MIN_A 4
#define RECALGO_AUTOINT_MAX_A 32        /* width of a head (A % 4 == 0) */
#define RECALGO_AUTOINT_MAX_H 4         /* heads */
#define RECALGO_AUTOINT_MAX_HA 64       /* output width H A of a layer */
#define RECALGO_AUTOINT_MAX_PARTIAL_ROWS 512

/* ------------------------------------------------------------------------------------------
 * One layer, per example.  x is [F, D]: the F field rows, each of input width D.  H heads of width A; output columns are
 * head-major, c = h A + a.
 *   Q_h = x Wq[h]      K_h = x Wk[h]      V_h = x Wv[h]          [F, A] each;  Wq, Wk, Wv: [H, D, A] contiguous
 *   S_h = Q_h K_h^T                                              [F, F], NO scaling (every field attends to all F, itself included)
 *   P_h = softmax(S_h) over the keys j, each row shifted by its maximum
 *   O   = concat_h (P_h V_h)                                     [F, H A]
 *   y   = relu(O + x Wres)                                       Wres [D, H A]; a NULL Wres means no residual term: y = relu(O)
 * No biases, no layer norm, no dropout.  Every product is a k-ordered fp32 fmaf chain (v_mfma_f32_16x16x4_f32).
 *
 *   x, dx      [B, F D] contiguous
 *   y, g       [B, F H A] contiguous
 *
 * backward (Q, K, V, S and P are recomputed from x; the ReLU mask is taken from y):
 *   dz = g * [y > 0]
 *   dWres = sum x^T dz                    dx  = dz Wres^T
 *   dV_h  = P_h^T dz_h                    dP_h = dz_h V_h^T
 *   dS_h  = P_h * (dP_h - rowsum(P_h * dP_h))
 *   dQ_h  = dS_h K_h                      dK_h = dS_h^T Q_h
 *   dx   += sum_h dQ_h Wq[h]^T + dK_h Wk[h]^T + dV_h Wv[h]^T
 *   dWq[h] = sum x^T dQ_h   (likewise dWk, dWv)         sums over the examples
 * dx, dwq, dwk, dwv and dwres are OVERWRITTEN.  A workgroup serves `waves` examples at a time (4, or 2 or 1 where the LDS of a
 * workgroup does not hold four examples' state) and leaves ONE partial row [dWq | dWk | dWv | dWres] of 3 H D A + D H A floats
 * (3 H D A without the residual term) in `workspace`: recalgo_autoint_bwd_partial_rows(B, F, D, A, H) =
 * min(ceil(B / waves), RECALGO_AUTOINT_MAX_PARTIAL_ROWS) rows, contiguous; recalgo_autoint_bwd_workspace_bytes = rows * the
 * row's floats * 4.  The gradients are the fixed-order sums of the rows (the order of recalgo_colsum_t, recalgo.h).  An
 * example's y and dx depend on that example alone: neither B nor its place in the batch changes a bit of them.
 *
 * Served (recalgo_autoint_supported): 2 <= F <= 64; 4 <= D <= 64 with D % 4 == 0; 4 <= A <= 32 with A % 4 == 0; 1 <= H <= 4
 * with H A <= 64; B >= 1.  An unsupported shape, B < 1, a NULL pointer (wres, and dwres with it, excepted), dwres given
 * without wres or the reverse, or a pointer that is not 4-byte aligned returns hipErrorInvalidValue and launches nothing; the
 * two queries return 0 for an unsupported shape or B < 1.
 * ------------------------------------------------------------------------------------------ */
int recalgo_autoint_supported(int F, int D, int A, int H);
int recalgo_autoint_bwd_partial_rows(int B, int F, int D, int A, int H);
int64_t recalgo_autoint_bwd_workspace_bytes(int B, int F, int D, int A, int H, int has_res);
int recalgo_autoint_layer_fwd(const float* x, const float* wq, const float* wk, const float* wv, const float* wres, int B, int F,
                              int D, int A, int H, float* y, recalgo_stream_t stream);
int recalgo_autoint_layer_bwd(const float* g, const float* x, const float* y, const float* wq, const float* wk, const float* wv,
                              const float* wres, int B, int F, int D, int A, int H, float* dx, float* dwq, float* dwk,
                              float* dwv, float* dwres, void* workspace, recalgo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECALGO_AUTOINT_H_ */
