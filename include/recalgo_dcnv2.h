/* recalgo_dcnv2.h — C-ABI header of librecalgo_hip.so for DCN-V2's cross layer (Wang et al., "DCN V2: Improved Deep & Cross
 * Network", WWW 2021, arXiv 2008.13535, eq. 4): the mixture of low-rank experts with a softmax gate, one entry each way.
 * Self-contained (it repeats the stream typedef: an identical typedef twice is valid C11 and C++); the conventions are those of
 * recalgo.h: hipError_t as int, device pointers, fp32, asynchronous on `stream`, no hidden allocation, no float atomics
 * (bit-reproducible, hipGraph-capturable).
 */
#ifndef RECALGO_DCNV2_H_
#define RECALGO_DCNV2_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* recalgo_stream_t; /* hipStream_t */

/* ABI version of THIS header; include/recalgo_dcnv2.abi records the hash of the declarations each version stands for. */
#define RECALGO_DCNV2_ABI_VERSION 1
int recalgo_dcnv2_abi_version(void);

#define RECALGO_DCNV2_MIN_D 4
#define RECALGO_DCNV2_MAX_D 512         /* width of x0 and xl (any D in the range) */
#define RECALGO_DCNV2_MIN_R 4
#define RECALGO_DCNV2_MAX_R 64          /* rank of an expert (r % 4 == 0) */
#define RECALGO_DCNV2_MAX_E 4           /* experts */
#define RECALGO_DCNV2_TILE 16           /* examples of one tile */
#define RECALGO_DCNV2_ROW_TILES 16      /* tiles a partial row covers before the cap on the rows holds */
#define RECALGO_DCNV2_MAX_PARTIAL_ROWS 64

/* ------------------------------------------------------------------------------------------
 * One layer, per example.  x0 and xl are rows of width D; E experts of rank r.
 *   V, U  [E, D, r]     C  [E, r, r]     gate  [E, D]     bias  [D] (shared by the experts)          all contiguous
 *   v_e = tanh(xl V_e)                    [r]
 *   c_e = tanh(v_e C_e)                   [r]
 *   u_e = c_e U_e^T + bias                [D]
 *   s_e = xl . gate_e                     no bias
 *   p   = softmax(s) over the E experts, shifted by its maximum
 *   y   = x0 * (sum_e p_e u_e) + xl
 * With E == 1, gate (and dgate with it) may be NULL: p = 1, the plain low-rank layer (eq. 3 with the nonlinearities in the
 * projected space).  Every product is a k-ordered fp32 fmaf chain (v_mfma_f32_16x16x4_f32); tanh and exp are the accurate
 * device-library functions.
 *
 *   x0, xl, y, g, dx0, dxl   [B, D] contiguous (a row start is 4-byte aligned, no more)
 *
 * backward (g = dL/dy; everything is recomputed from x0, xl and the weights):
 *   m = sum_e p_e u_e         dx0 = g * m         q = g * x0          dbias = sum q
 *   dp_e = q . u_e            ds_e = p_e (dp_e - sum_e' p_e' dp_e')    du_e = p_e q
 *   dU_e = sum du_e^T c_e     dcpre_e = (du_e U_e) * (1 - c_e^2)       dC_e = sum v_e^T dcpre_e
 *   dvpre_e = (dcpre_e C_e^T) * (1 - v_e^2)       dV_e = sum xl^T dvpre_e            dgate_e = sum ds_e xl
 *   dxl = g + sum_e ds_e gate_e + sum_e dvpre_e V_e^T                  (sums without an index run over the examples)
 * dx0, dxl and the five parameter gradients are OVERWRITTEN; dx0 and dxl are separate outputs (where xl IS x0 the caller adds
 * them).  An example's y, dx0 and dxl depend on that example alone: neither B nor its place in the batch changes a bit of them.
 *
 * The weight gradients do not fit a workgroup's registers (E 2 D r accumulators), so the backward runs in two launches and a
 * fixed-order sum.  `workspace`, in floats, R = recalgo_dcnv2_bwd_partial_rows(B, D, r, E), ROW = E (2 D r + r^2 + D) + D:
 *   [0, R ROW)                     the partial rows, see below
 *   then, per example, contiguous: pc [B, E r] = p_e c_e,  dvpre [B, E r],  v [B, E r],  dcpre [B, E r],  ds [B, 4]
 *   (expert-major columns e r + k; ds holds zeros from column E on)
 * recalgo_dcnv2_bwd_workspace_bytes = 4 (R ROW + B (4 E r + 4)).  The first launch writes dx0, dxl and the per-example part;
 * the second forms the partial rows from it, x0, xl and g: with T = ceil(B / 16) tiles of 16 examples,
 * R = min(ceil(T / RECALGO_DCNV2_ROW_TILES), RECALGO_DCNV2_MAX_PARTIAL_ROWS) and row s sums the examples of the tiles
 * [s T / R, (s + 1) T / R) (integer division) in example order.  A row is [dV | dC | dU | dgate | dbias], ROW floats; without
 * a gate the dgate part is absent and the rows are ROW - D floats apart.  The gradients are the fixed-order sums of the rows (the
 * order of recalgo_colsum_t, recalgo.h).  There is no [B, E, D] tensor anywhere.
 *
 * Served (recalgo_dcnv2_supported): 4 <= D <= 512; 4 <= r <= 64 with r % 4 == 0; 1 <= E <= 4; B >= 1.  An unsupported shape,
 * B < 1, a NULL pointer (gate and dgate with E == 1 excepted), gate given without dgate or the reverse, or a pointer that is not
 * 4-byte aligned returns hipErrorInvalidValue and launches nothing; the queries return 0 for an unsupported shape or B < 1.
 * ------------------------------------------------------------------------------------------ */
int recalgo_dcnv2_supported(int D, int r, int E);
int recalgo_dcnv2_bwd_partial_rows(int B, int D, int r, int E);
int64_t recalgo_dcnv2_bwd_workspace_bytes(int B, int D, int r, int E);
int recalgo_dcnv2_layer_fwd(const float* x0, const float* xl, const float* V, const float* C, const float* U, const float* gate,
                            const float* bias, int B, int D, int r, int E, float* y, recalgo_stream_t stream);
int recalgo_dcnv2_layer_bwd(const float* g, const float* x0, const float* xl, const float* V, const float* C, const float* U,
                            const float* gate, const float* bias, int B, int D, int r, int E, float* dx0, float* dxl, float* dV,
                            float* dC, float* dU, float* dgate, float* dbias, void* workspace, recalgo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECALGO_DCNV2_H_ */
