/* recalgo_serve.h — seventh C-ABI header of librecalgo_hip.so: inference-only kernels of the serving path
 * (recalgorithm_amd/export.py ServingModel.compile).  The hidden MLP tower of a small request as ONE launch: up to four
 * dense(relu) -> [dropout = identity] -> [BatchNorm inference] layers (algorithm/DeepFM/deepfm.py:207-211, the same block in NFM,
 * PNN, Wide&Deep and xDeepFM; DCN's plain dense(relu) stack), the BatchNorm folded by the caller into one scale and one shift
 * per column.  Self-contained (it repeats the stream typedef: an identical typedef twice is valid C11 and C++); the conventions
 * are those of recalgo.h: hipError_t as int, device pointers except the short HOST tables, fp32, asynchronous on `stream`, no
 * hidden allocation, no atomics (bit-reproducible, hipGraph-capturable).
 */
#ifndef RECALGO_SERVE_H_
#define RECALGO_SERVE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* recalgo_stream_t; /* hipStream_t */

/* ABI version of THIS header; include/recalgo_serve.abi records the hash of the declarations each version stands for. */
#define RECALGO_SERVE_ABI_VERSION 1
int recalgo_serve_abi_version(void);

#define RECALGO_SERVE_MAX_LAYERS 4
#define RECALGO_SERVE_MAX_IN 1024   /* K0, any value >= 1 */
#define RECALGO_SERVE_MAX_UNITS 512 /* each hidden width, % 16 == 0, >= 16 */

/* ------------------------------------------------------------------------------------------
 * With h_0 = x [B, K0], K_0 = K0 and K_l = units[l - 1], for l = 0 .. L-1:
 *   z       = h_l W_l + b_l              W_l [K_l, units[l]] row-major; b[l] == NULL (or b == NULL): no bias
 *   a       = relu(z) if bit l of relu_bits is set, else z
 *   h_{l+1} = fmaf(a, scale_l, shift_l)  per column; scale[l] == NULL (or scale == NULL): h_{l+1} = a, shift[l] is not read
 *   out     = h_L [B, units[L-1]]
 * The caller folds a BatchNorm once: scale = gamma * rsqrt(moving_variance + epsilon), shift = beta - moving_mean * scale.
 *
 * The order of every dot product.  z[row][col] = c0 + c1, two fp32 fmaf chains (the matrix unit's 16x16x4 fp32 step is an fmaf
 * chain): c0 starts at b_l[col] (0 without a bias), c1 at 0.  The terms h_l[row][k] * W_l[k][col] are taken in groups of 16
 * consecutive k; group g = k / 16 goes to chain g % 2, groups in ascending order; inside a group the order is
 *   for x = 0 .. 3: for q = 0 .. 3: k = 16 g + 4 q + x
 * and a last group that reaches past K_l ends with exact zero terms.  Nothing else is added, nothing is reassociated.
 * A row's result depends on that row alone: neither B nor the row's place in the batch changes a bit of it.
 *
 *   x       [B, K0] contiguous          out  [B, units[L-1]] contiguous
 *   w, b, scale, shift   HOST arrays of L device pointers (b, scale, shift: or NULL = every entry NULL); units HOST array of L
 *
 * Served (recalgo_serve_tower_supported): 1 <= L <= 4, 1 <= K0 <= 1024, every units[l] in 16 .. 512 with units[l] % 16 == 0;
 * B >= 1.  An unsupported shape, a NULL x, out, w, units or w[l], a scale[l] without its shift[l], or a pointer that is not
 * 4-byte aligned returns hipErrorInvalidValue and launches nothing.  (x moves as 16-byte accesses when K0 % 4 == 0 and x is
 * 16-byte aligned, as 4-byte ones otherwise; the results are the same bits.)
 *
 * One workgroup per 16 rows, each streaming the whole weight set from L2: a latency chain whose time hardly moves with B up to
 * one workgroup per compute unit (bench widths 416 -> 512 -> 256 -> 128: 51 us at B = 1, 53 us at B = 4096).  Measured against
 * the launches it replaces (profiles/serving_bench.json): faster than three dense launches plus three inference BatchNorms at
 * every size from 1 to 4096 rows, slower than three dense launches alone at every size; past 4096 rows it is not measured.
 * ------------------------------------------------------------------------------------------ */
int recalgo_serve_tower_supported(int K0, const int* units, int L);
int recalgo_serve_tower_fwd(const float* x, const float* const* w, const float* const* b, const float* const* scale,
                            const float* const* shift, const int* units, int L, unsigned relu_bits, int B, int K0, float* out,
                            recalgo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECALGO_SERVE_H_ */
