/* recalgo_sumstep.h — ninth C-ABI header of librecalgo_hip.so: the step's deferred gradient sums and the dense optimizer
 * update as ONE launch.  Self-contained (it repeats the stream typedef: an identical typedef twice is valid C11 and C++); the
 * descriptor arrays are those of recalgo.h and are declared `const void*` here, each with the type it points to.  The
 * conventions are those of recalgo.h: hipError_t as int, asynchronous on `stream`, no hidden allocation, no host read-back
 * (hipGraph-capturable), descriptor arrays are HOST arrays read at launch time.
 */
#ifndef RECALGO_SUMSTEP_H_
#define RECALGO_SUMSTEP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* recalgo_stream_t; /* hipStream_t */

/* ABI version of THIS header; include/recalgo_sumstep.abi records the hash of the declarations each version stands for. */
#define RECALGO_SUMSTEP_ABI_VERSION 1
int recalgo_sumstep_abi_version(void);

/* recalgo_dense_bwd_weights_reduce(jobs, n_jobs, sums, n_sums, step_dev) followed by recalgo_adam_tf1_step_plans(.., advance = 0, ..)
 * (both recalgo.h) as ONE launch, bit-identical to the two (p, m, v, the gradient buffer, the counter): the thread that updates a
 * parameter sums its gradient's slabs / partial rows itself, in the order of the sum launch, instead of reading the sum back
 * from g.  What g holds afterwards is what the two launches leave (the sums, or zeros with zero_grad); elements of [g, g + n)
 * that no job writes take their gradient from g.  Every argument up to n_scans is that of recalgo_adam_tf1_step_plans, and:
 *   arenas           const recalgo_adam_arena_t[n_arenas]
 *   scans            const recalgo_plan_scan_t[n_scans]
 *   jobs, sums       const recalgo_dense_split_t[n_jobs], const recalgo_colsum_t[n_sums]: the arrays of
 *                    recalgo_dense_bwd_weights_reduce; every output (dw, dbias, out) must lie inside [g, g + n)
 *   side_sums        const recalgo_colsum_t[n_side_sums]: column sums whose outputs are NOT gradients of the flat buffer (the loss
 *                    value): only summed; every output must lie outside [g, g + n)
 *   advance          as recalgo_adam_tf1_step (a training step passes 1: no other launch advances the counter)
 *   ticket_dev       a workspace of recalgo_adam_tf1_sum_step_workspace_bytes() bytes, as ints (required with advance != 0), zero
 *                    before the first call and the launch's own from then on: the arrival ticket, sharded over words on lines of
 *                    their own (hundreds of workgroups arrive together; every call leaves those words zero), and behind them lr_t
 *                    of the step to come, which an extra workgroup computes beside the update so that the next call need not
 *                    (it compares t, lr and the betas)
 * recalgo_adam_tf1_sum_step_supported -> 1, or 0 when the launch cannot serve the jobs: an output on the wrong side of the flat
 * buffer's bounds, two overlapping outputs, a descriptor recalgo_dense_bwd_weights_reduce would refuse, n > 0 with g not 16-byte
 * aligned, or more than 32 jobs (sums + side_sums + the jobs whose shape has more than one split; the job table travels in the
 * kernel arguments).  recalgo_adam_tf1_sum_step then returns hipErrorInvalidValue and launches nothing: run the two launches. */
int64_t recalgo_adam_tf1_sum_step_workspace_bytes(void);
int recalgo_adam_tf1_sum_step_supported(const float* g, int64_t n, const void* jobs, int n_jobs, const void* sums, int n_sums,
                                        const void* side_sums, int n_side_sums);
int recalgo_adam_tf1_sum_step(float* p, float* g, float* m, float* v, int64_t n, const void* arenas, int n_arenas,
                              int64_t* step_dev, int* ticket_dev, int advance, float lr, float beta1, float beta2, float eps,
                              int zero_grad, const void* scans, int n_scans, const void* jobs, int n_jobs, const void* sums,
                              int n_sums, const void* side_sums, int n_side_sums, recalgo_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* RECALGO_SUMSTEP_H_ */
