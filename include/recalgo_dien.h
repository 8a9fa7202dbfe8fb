/* recalgo_dien.h — C-ABI header of librecalgo_hip.so for DIEN's interest module (algorithm/DIEN/dien.py:196-229,
 * custom_grucell.py): the GRU recurrence, and attention + the AGRU / AUGRU recurrence, two launches each way.  Self-contained
 * (it repeats the stream typedef: an identical typedef twice is valid C11 and C++); the conventions are those of recalgo.h:
 * hipError_t as int, device pointers, fp32, asynchronous on `stream`, no hidden allocation, no float atomics
 * (bit-reproducible, hipGraph-capturable).
 */
#ifndef RECALGO_DIEN_H_
#define RECALGO_DIEN_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* recalgo_stream_t; /* hipStream_t */

/* ABI version of THIS header; include/recalgo_dien.abi records the hash of the declarations each version stands for. */
#define RECALGO_DIEN_ABI_VERSION 1
int recalgo_dien_abi_version(void);

#define RECALGO_DIEN_MAX_T 64  /* steps of one example */
#define RECALGO_DIEN_MAX_NA 16 /* width of a step's input row (na % 4 == 0) */
#define RECALGO_DIEN_MAX_NH 16 /* units of the state (nh % 4 == 0) */

#define RECALGO_DIEN_MODE_GRU 0
#define RECALGO_DIEN_MODE_AGRU 1
#define RECALGO_DIEN_MODE_AUGRU 2

/* ------------------------------------------------------------------------------------------
 * The cell (TF 1.14's GRUCell arithmetic, shared by the three modes); x_t [nx], state h [nh], Wg [nx + nh, 2 nh],
 * bg [2 nh], Wc [nx + nh, nh], bc [nh], all row-major:
 *   [r, u] = sigmoid([x_t, h] Wg + bg)        r = the first nh columns, u = the last nh
 *   c      = tanh([x_t, r * h] Wc + bc)       the reset gate is applied BEFORE the product
 *   GRU   (mode 0): h' = u h + (1 - u) c
 *   AGRU  (mode 1): h' = (1 - a_t) h + a_t c            (u is unused: the u half of dWg and dbg is exactly zero)
 *   AUGRU (mode 2): u' = (1 - a_t) u;  h' = u' h + (1 - u') c
 * The state starts at zero.  L = lengths[b] clamped to [0, T] (lengths == NULL where it is optional: L = T): for t >= L the
 * state is copied through and the output row is zero; what the input rows t >= L hold never reaches a result.
 *
 * gru (mode 0, nx = na):    x [B, T, na] -> h [B, T, nh].  gru_bwd recomputes the gates of step t from x[t] and h[t - 1]
 *   (nothing but h is saved), takes g_h [B, T, nh] (rows t >= L are not read) and writes dx [B, T, na] (rows t >= L zero)
 *   and the four parameter gradients.
 * evolve (mode 1 or 2, nx = nh; the cell's Wg is [2 nh, 2 nh], Wc [2 nh, nh]):  h [B, T, nh], target [B, na],
 *   w_att [nh, na], lengths (required):
 *     e_b = w_att target_b;   s[b, t] = h[b, t] . e_b, REPLACED by -4294967296.0f for t >= L;
 *     att[b, :] = softmax over all T entries (max-subtracted; a replaced entry contributes exactly 0.0f, L = 0 gives 1 / T);
 *     states [B, T, nh] = the recurrence over the rows of h with a_t = att[b, t];  final_state [B, nh] = the state after step L - 1
 *     (zeros for L = 0).
 *   evolve_bwd takes the forward's inputs and outputs and g_final [B, nh]; dh [B, T, nh] = the cell-input path plus the
 *   score path (rows t >= L zero), dtarget [B, na], dw_att [nh, na] and the four cell gradients.
 *
 * Parameter gradients, two passes: workgroup r of the backward grid (rows = recalgo_dien_*_bwd_partial_rows(B) = min(B, 256)
 * workgroups) takes the examples r, r + rows, r + 2 rows, ..; it adds them in that order, the steps of an example from the
 * last to the first, and writes ONE row of `workspace` (recalgo_dien_*_bwd_workspace_bytes):
 *   gru:     [rows][ dWg (na + nh) 2 nh | dbg 2 nh | dWc (na + nh) nh | dbc nh ]                       floats
 *   evolve:  [rows][ dw_att nh na | dWg 2 nh 2 nh | dbg 2 nh | dWc 2 nh nh | dbc nh ]                  floats
 * the same entry then sums the rows column-wise in a fixed order: sixteen interleaved sums (rows g, g + 16, g + 32, .. in
 * that order, g = 0..15), then those sixteen in the order of g.  Two runs on the same inputs are bit-equal.
 *
 * Served (recalgo_dien_supported; anything else, B < 1, a mode other than the entry's, a NULL pointer other than the
 * optional `lengths` of the gru entries, or a pointer that is not 4-byte aligned returns hipErrorInvalidValue and launches
 * nothing): 1 <= T <= 64, na in {4, 8, 12, 16}, nh in {4, 8, 12, 16}.
 * ------------------------------------------------------------------------------------------ */
int recalgo_dien_supported(int T, int na, int nh);
int recalgo_dien_gru_bwd_partial_rows(int B);
int64_t recalgo_dien_gru_bwd_workspace_bytes(int B, int na, int nh);
int recalgo_dien_evolve_bwd_partial_rows(int B);
int64_t recalgo_dien_evolve_bwd_workspace_bytes(int B, int na, int nh);
int recalgo_dien_gru_fwd(const float* x, const int32_t* lengths, const float* Wg, const float* bg, const float* Wc,
                         const float* bc, int B, int T, int na, int nh, float* h, recalgo_stream_t stream);
int recalgo_dien_gru_bwd(const float* x, const int32_t* lengths, const float* h, const float* Wg, const float* bg,
                         const float* Wc, const float* bc, const float* g_h, int B, int T, int na, int nh, float* dx, float* dWg,
                         float* dbg, float* dWc, float* dbc, float* workspace, recalgo_stream_t stream);
int recalgo_dien_evolve_fwd(const float* h, const float* target, const int32_t* lengths, const float* w_att, const float* Wg,
                            const float* bg, const float* Wc, const float* bc, int B, int T, int na, int nh, int mode,
                            float* att, float* states, float* final_state, recalgo_stream_t stream);
int recalgo_dien_evolve_bwd(const float* h, const float* target, const int32_t* lengths, const float* w_att, const float* Wg,
                            const float* bg, const float* Wc, const float* bc, const float* att, const float* states,
                            const float* g_final, int B, int T, int na, int nh, int mode, float* dh, float* dtarget,
                            float* dw_att, float* dWg, float* dbg, float* dWc, float* dbc, float* workspace,
                            recalgo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECALGO_DIEN_H_ */
