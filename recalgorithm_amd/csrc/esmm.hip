// ESMM's loss tail (include/recalgo_esmm.h): the click loss, the entire-space click-and-conversion loss, their sum, the three
// probabilities and both logit gradients in ONE launch.
//   * one 1024-thread workgroup, as sigmoid_ce_kernel (csrc/tail.hip) and multitask_sigmoid_ce_kernel (csrc/mmoe.hip): the click
//     half IS sigmoid_ce_task (sigmoid_ce.h), so its loss, probabilities and gradient are that kernel's bits — the order in which
//     it adds the rows (thread t: rows t, t + 1024, ..; a wave sum; 16 wave results) is part of that, and a grid of workgroups
//     could not keep it.  The tail is a latency link of the step's chain (B = 4096: four rows per thread), not a throughput
//     kernel; the second term rides in the same pass over the rows, inside the callbacks sigmoid_ce_task makes per row, and its
//     sum is reduced the same way behind it;
//   * the second term is evaluated in logit space (the header states the arithmetic): log p and log(1 - p) come from softplus
//     and a three-way logsumexp, the gradients from exp of differences of those — 1 - p is never formed;
//   * no atomics, plain C++ stores; a thread reads and writes only its own rows until the two reductions.
#include "common.h"
#include "sigmoid_ce.h"
#include "../../include/recalgo_esmm.h"

namespace {

__global__ __launch_bounds__(1024) void esmm_loss_kernel(const float* __restrict__ ctr_logit, const float* __restrict__ cvr_logit,
                                                         const float* __restrict__ click, const float* __restrict__ conversion,
                                                         unsigned B, float grad_scale, float* __restrict__ prob,
                                                         float* __restrict__ losses, float* __restrict__ total,
                                                         float* __restrict__ d_ctr, float* __restrict__ d_cvr) {
    __shared__ float red[16];
    __shared__ float red2[16];
    const bool want = d_ctr != nullptr;
    const float gscale = grad_scale * (1.0f / (float)B);
    float acc2 = 0.f;        // this thread's rows of the second term, in row order
    float ga = 0.f, gb = 0.f;  // dl/da, dl/db of the row in flight: set by the first callback, stored by the second

    const float l_ctr = sigmoid_ce_task(
        ctr_logit, click, B, grad_scale, want, red,
        [&](unsigned i, float p_ctr) {
            const float a = ctr_logit[i], b = cvr_logit[i];
            const float z = click[i] * conversion[i];
            const float eb = expf(-fabsf(b));
            const float r = eb / (1.0f + eb);
            const float p_cvr = b >= 0.f ? 1.0f / (1.0f + eb) : r;
            float* const row = prob + (size_t)i * 3;
            row[0] = p_ctr;
            row[1] = p_cvr;
            row[2] = p_ctr * p_cvr;
            // sp(x) and sp(-x) share log1p(exp(-|x|))
            const float la = log1pf(expf(-fabsf(a))), lb = log1pf(eb);
            const float sp_a = fmaxf(a, 0.f) + la, sp_na = fmaxf(-a, 0.f) + la;
            const float sp_b = fmaxf(b, 0.f) + lb, sp_nb = fmaxf(-b, 0.f) + lb;
            const float log_p = -sp_na - sp_nb;
            const float t0 = -a, t1 = -b, t2 = -a - b;
            const float m = fmaxf(fmaxf(t0, t1), t2);
            const float lam = m + logf(expf(t0 - m) + expf(t1 - m) + expf(t2 - m));
            const float log_1mp = lam + log_p;
            acc2 += -z * log_p - (1.0f - z) * log_1mp;
            if (want) {
                ga = (1.0f - z) * expf(-sp_a - lam) - z * expf(-sp_a);
                gb = (1.0f - z) * expf(-sp_b - lam) - z * expf(-sp_b);
            }
        },
        [&](unsigned i, float d) {
            d_ctr[i] = d + ga * gscale;
            d_cvr[i] = gb * gscale;
        });

    acc2 = wave_sum(acc2);
    if ((threadIdx.x & 63) == 0) red2[threadIdx.x >> 6] = acc2;
    __syncthreads();
    if (threadIdx.x < 64) {
        float v = threadIdx.x < 16 ? red2[threadIdx.x] : 0.f;
        v = wave_sum(v);
        if (threadIdx.x == 0) {
            // total is the sum of the two values AS STORED: the mean is rounded before it is added (no fused multiply-add)
#pragma clang fp contract(off)
            const float l_ctcvr = v * (1.0f / (float)B);
            losses[0] = l_ctr;
            losses[1] = l_ctcvr;
            total[0] = l_ctr + l_ctcvr;
        }
    }
}

}  // namespace

RECALGO_EXPORT int recalgo_esmm_abi_version(void) { return RECALGO_ESMM_ABI_VERSION; }

RECALGO_EXPORT int recalgo_esmm_loss_fwd_bwd(const float* ctr_logit, const float* cvr_logit, const float* click,
                                             const float* conversion, int B, float grad_scale, float* prob, float* losses,
                                             float* total, float* d_ctr_logit, float* d_cvr_logit, recalgo_stream_t stream) {
    RECALGO_REQUIRE(B >= 1 && B <= RECALGO_ESMM_MAX_ROWS);
    RECALGO_REQUIRE(ctr_logit && cvr_logit && click && conversion && prob && losses && total);
    RECALGO_REQUIRE((d_ctr_logit == nullptr) == (d_cvr_logit == nullptr));
    RECALGO_REQUIRE(aligned_to<4>(ctr_logit, cvr_logit, click, conversion) && aligned_to<4>(prob, losses, total, d_ctr_logit, d_cvr_logit));
    hipLaunchKernelGGL(esmm_loss_kernel, dim3(1), dim3(1024), 0, as_stream(stream), ctr_logit, cvr_logit, click, conversion,
                       (unsigned)B, grad_scale, prob, losses, total, d_ctr_logit, d_cvr_logit);
    RECALGO_RETURN_LAST();
}
