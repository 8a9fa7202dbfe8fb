/* recalgo_cgc.h — second C-ABI header of librecalgo_hip.so: the "customized gate control" (CGC) block of PLE
 * (algorithm/PLE/extraction_network.py:25-85, algorithm/PLE/ple.py:185-226), at sizes beyond recalgo_gate_mix_* of
 * recalgo.h.  Self-contained (it repeats the stream typedef: an identical typedef twice is valid C11 and C++); the
 * conventions are those of recalgo.h: hipError_t as int, device pointers except the short HOST pointer tables, fp32,
 * asynchronous on `stream`, no hidden allocation, no float atomics (bit-reproducible, hipGraph-capturable).
 */
#ifndef RECALGO_CGC_H_
#define RECALGO_CGC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* recalgo_stream_t; /* hipStream_t */

/* ABI version of THIS header; include/recalgo_cgc.abi records the hash of the declarations each version stands for. */
#define RECALGO_CGC_ABI_VERSION 1
int recalgo_cgc_abi_version(void);

#define RECALGO_CGC_MAX_EXPERTS 32 /* E, and the experts one gate selects (n_g) */
#define RECALGO_CGC_MAX_GATES 8    /* G */

/* ------------------------------------------------------------------------------------------
 * CGC: G bias-free softmax gates over ONE input and the mix of E expert outputs by a selection table, one kernel each
 * way.  With c[g][e] = sum_{j: sel[g][j] = e} p_g[j]:
 *   z_g = x Wg            p_g = softmax(z_g)       (max-subtracted; logits and softmax evaluated in double)
 *   sum_outputs == 0:  outs[g] = sum_e c[g][e] * experts[e]                  G outputs   (ple.py:215-226)
 *   sum_outputs != 0:  outs[0] = sum_e (sum_g c[g][e]) * experts[e]          ONE output  (extraction_network.py:85,
 *                                                                             tf.add_n of the task and all-gate outputs)
 * backward (d = d_outs[g], or the one d_outs[0] shared by every gate when sum_outputs):
 *   d_experts[e] = sum_g c[g][e] * d_g   (zeroed where experts[e] <= 0 when relu_experts)
 *   dp_g[j] = <d_g, experts[sel[g][j]]>      dz_g = p_g * (dp_g - sum_j p_g[j] dp_g[j])
 *   dx = sum_g dz_g Wg^T                     dWg = x^T dz_g
 *
 *   x            [B, ldx] (ldx >= In)
 *   gate_kernels HOST array of G device pointers, gate g: [In, n_sel[g]] row-major
 *   n_sel        HOST [G]; sel HOST [sum n_sel] expert indices in [0, E), gate after gate (duplicates allowed)
 *   experts      HOST array of E device pointers, each [B, H] contiguous
 *   outs         HOST array of G (sum_outputs: 1) device pointers [B, H]
 *   p            [B, sum n_sel] the gate probabilities (written by fwd, read by bwd)
 *   d_outs       HOST array of G (sum_outputs: 1) device pointers [B, H] contiguous; a NULL entry (sum_outputs == 0
 *                only): that gate gets no gradient
 *   d_experts    HOST array of E device pointers [B, H], or NULL; a NULL entry: that gradient is not wanted
 *   dx           [B, lddx] or NULL
 *   partials     [recalgo_cgc_partial_rows(B, In, sum n_sel)][In * sum n_sel]: per-workgroup sums of x^T dz_g; gate g's
 *                [In, n_sel[g]] gradient is the run that starts at column In * (n_sel[0] + .. + n_sel[g-1]).  The caller
 *                sums the rows in order (recalgo_dense_bwd_weights_reduce).
 * Served (recalgo_cgc_supported, n_total = sum n_sel, n_max = max n_sel; anything else returns hipErrorInvalidValue and
 * launches nothing): H >= 4, H % 4 == 0, 1 <= E <= 32, 1 <= G <= 8, 1 <= n_g <= 32, 1 <= In <= 512,
 * In * (n_total | 1) <= 20480 floats (the gate kernels are staged in 80 KiB of LDS), B >= 1.
 * Experts, outputs and gradients whose base pointers are all 16-byte aligned take the float4 arm, anything else the
 * scalar-access arm of the same kernels.
 * ------------------------------------------------------------------------------------------ */
int recalgo_cgc_supported(int In, int E, int G, int H, int n_total, int n_max);
int recalgo_cgc_partial_rows(int B, int In, int n_total);
int recalgo_cgc_fwd(const float* x, int ldx, const float* const* gate_kernels, const int* n_sel, const int* sel,
                    const float* const* experts, int B, int In, int E, int G, int H, int sum_outputs,
                    float* const* outs, float* p, recalgo_stream_t stream);
int recalgo_cgc_bwd(const float* x, int ldx, const float* const* gate_kernels, const int* n_sel, const int* sel,
                    const float* const* experts, const float* p, const float* const* d_outs, int B, int In, int E,
                    int G, int H, int sum_outputs, int relu_experts, float* const* d_experts, float* dx, int lddx,
                    float* partials, recalgo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECALGO_CGC_H_ */
