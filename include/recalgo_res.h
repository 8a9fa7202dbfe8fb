/* recalgo_res.h — fifth C-ABI header of librecalgo_hip.so: the residual stack of DeepCrossing
 * (algorithm/DeepCrossing/residual_unit.py:4-22, deepcrossing.py:154-157), one kernel each way for the whole stack.
 * Self-contained (it repeats the stream typedef: an identical typedef twice is valid C11 and C++); the conventions are those
 * of recalgo.h: hipError_t as int, device pointers except the short HOST pointer tables, fp32, asynchronous on `stream`, no
 * hidden allocation, no float atomics (bit-reproducible, hipGraph-capturable).
 */
#ifndef RECALGO_RES_H_
#define RECALGO_RES_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* recalgo_stream_t; /* hipStream_t */

/* ABI version of THIS header; include/recalgo_res.abi records the hash of the declarations each version stands for. */
#define RECALGO_RES_ABI_VERSION 1
int recalgo_res_abi_version(void);

#define RECALGO_RES_MAX_D 512   /* width of the stack's input and of every unit's output */
#define RECALGO_RES_MAX_H 256   /* internal width of a unit (H % 16 == 0, H >= 16) */
#define RECALGO_RES_MAX_UNITS 8 /* L */

/* ------------------------------------------------------------------------------------------
 * A stack of L residual units over the rows of x; with x_0 = x, for l = 0 .. L-1:
 *   h_l     = relu(x_l W0_l + b0_l)              W0_l [D, H] row-major, b0_l [H]
 *   x_{l+1} = relu(x_l + (h_l W1_l + b1_l))      W1_l [H, D] row-major, b1_l [D]
 * Every dot product is eight k-ordered fp32 fmaf chains from 0 (the terms k = 4 s .. 4 s + 3 in chain s % 8) added pairwise in a
 * fixed order; the bias and the residual are added after it.
 *
 *   x, g, dx      [B, D] contiguous
 *   w0, b0, w1, b1  HOST arrays of L device pointers
 *   hs            [L, B, H]: hs[l] = h_l          (save != 0; NULL otherwise)
 *   ys            save != 0: [L, B, D], ys[l] = x_{l+1} (the last slab is the result); save == 0: [B, D], the result only
 *
 * backward, with g_L = g, for l = L-1 .. 0 (the masks are READ from the saved arrays: nothing is recomputed, the result is
 * a pure function of the arguments):
 *   dz_l = g_{l+1} * [ys[l] > 0]          dh_l = (dz_l W1_l^T) * [hs[l] > 0]          g_l = dz_l + dh_l W0_l^T
 *   dzs [L, B, D], dhs [L, B, H] (both masked: exactly 0.0 under a zero mask), dx = g_0.
 * The parameter gradients are batch sums the caller forms from them (recalgo_dense_bwd_weights of recalgo.h):
 *   dW0_l = x_l^T dh_l, db0_l = colsum(dh_l), dW1_l = h_l^T dz_l, db1_l = colsum(dz_l)       (x_0 = x, x_l = ys[l-1]).
 * A row's results depend on that row alone: neither B nor a row's place in the batch changes a bit of them.
 *
 * Served (recalgo_res_supported): 1 <= D <= 512, 16 <= H <= 256 with H % 16 == 0, 1 <= L <= 8; B >= 1.  An unsupported
 * shape, a NULL pointer (table entries included; hs only when save != 0), or a pointer that is not 4-byte aligned returns
 * hipErrorInvalidValue and launches nothing.  With D % 4 == 0 and x, hs, ys (g, dzs, dhs, dx) 16-byte aligned the row tiles
 * move as 16-byte accesses, anything else takes the 4-byte arm of the same kernels; the results are the same bits.
 * ------------------------------------------------------------------------------------------ */
int recalgo_res_supported(int D, int H, int L);
int recalgo_res_stack_fwd(const float* x, const float* const* w0, const float* const* b0, const float* const* w1,
                          const float* const* b1, int B, int D, int H, int L, int save, float* hs, float* ys,
                          recalgo_stream_t stream);
int recalgo_res_stack_bwd(const float* g, const float* hs, const float* ys, const float* const* w0, const float* const* w1,
                          int B, int D, int H, int L, float* dzs, float* dhs, float* dx, recalgo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECALGO_RES_H_ */
