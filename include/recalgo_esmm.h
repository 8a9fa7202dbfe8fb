/* recalgo_esmm.h — C-ABI header of librecalgo_hip.so for the loss tail of ESMM (Ma et al., SIGIR 2018, "Entire Space Multi-Task
 * Model"): the click loss and the entire-space click-and-conversion loss over ALL impressions, their sum, the three
 * probabilities and both logit gradients, as ONE launch (recalgorithm_amd/ops.py esmm_loss, model_tail.finish_esmm_model_fn).
 * Self-contained (it repeats the stream typedef: an identical typedef twice is valid C11 and C++); the conventions are those of
 * recalgo.h: hipError_t as int, device pointers, fp32, asynchronous on `stream`, no hidden allocation, no host read-back
 * (hipGraph-capturable).  Every sum over the rows is taken in one fixed order by one workgroup, without float atomics: the
 * results are bit-reproducible run to run.
 *
 * The arithmetic, for a row with CTR logit a, CVR logit b, click y and conversion c, all in fp32:
 *   sp(x)    = max(x, 0) + log1p(exp(-|x|))                    (softplus)
 *   z        = y * c                                            (a conversion without a click counts as none)
 *   L_ctr    = mean over the rows of  max(a, 0) - a y + log1p(exp(-|a|))   — recalgo_sigmoid_ce_fwd_bwd's value, bit for bit,
 *              with its probabilities pCTR = sigmoid(a) and its gradient (the same device function evaluates them)
 *   pCVR     = sigmoid(b), in the same two-branch form;  pCTCVR = pCTR * pCVR, the fp32 product of the two stored values
 *   log p    = -sp(-a) - sp(-b)                                 (p = sigmoid(a) sigmoid(b), never formed for the loss)
 *   Lambda   = logsumexp(-a, -b, -a - b), the maximum subtracted
 *   log(1-p) = Lambda + log p
 *   l        = -z log p - (1 - z) log(1-p);   L_ctcvr = mean over the rows of l
 *   dl/da    = (1 - z) exp(-sp(a) - Lambda) - z exp(-sp(a))
 *   dl/db    = (1 - z) exp(-sp(b) - Lambda) - z exp(-sp(b))
 * 1 - p and p / (1 - p) are never formed from probabilities: in fp32 1 - p rounds to 0 once both logits are large, and the loss
 * composed in probability space is then inf.  In this form every output is finite for |a|, |b| <= 30 at least.
 */
#ifndef RECALGO_ESMM_H_
#define RECALGO_ESMM_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* recalgo_stream_t; /* hipStream_t */

/* ABI version of THIS header; include/recalgo_esmm.abi records the hash of the declarations each version stands for. */
#define RECALGO_ESMM_ABI_VERSION 1
int recalgo_esmm_abi_version(void);

#define RECALGO_ESMM_MAX_ROWS 16777216 /* B: 1 .. 2^24 (one workgroup walks the rows; a float holds every B up to here exactly) */

/* ------------------------------------------------------------------------------------------
 * recalgo_esmm_loss_fwd_bwd — forward and backward in one launch of one 1024-thread workgroup.
 *   ctr_logit, cvr_logit, click, conversion   [B] each, contiguous
 *   prob          [B, 3] row-major: pCTR, pCVR, pCTCVR
 *   losses        [2]: L_ctr, L_ctcvr
 *   total         [1]: losses[0] + losses[1], added in that order
 *   d_ctr_logit   [B]: (d L_ctr / da as recalgo_sigmoid_ce_fwd_bwd gives it for grad_scale, B) + dl/da * grad_scale / B
 *   d_cvr_logit   [B]: dl/db * grad_scale / B
 *                 both NULL: forward only (losses, total and prob are the same bits); exactly one NULL: refused
 * The outputs may not overlap the inputs or each other.
 *
 * Refused with hipErrorInvalidValue before any launch: B < 1 or B > RECALGO_ESMM_MAX_ROWS; a NULL ctr_logit, cvr_logit, click,
 * conversion, prob, losses or total; exactly one of the two gradients NULL; a pointer that is not 4-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int recalgo_esmm_loss_fwd_bwd(const float* ctr_logit, const float* cvr_logit, const float* click, const float* conversion, int B,
                              float grad_scale, float* prob, float* losses, float* total, float* d_ctr_logit, float* d_cvr_logit,
                              recalgo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECALGO_ESMM_H_ */
