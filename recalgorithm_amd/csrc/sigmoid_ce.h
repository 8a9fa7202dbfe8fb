// The sigmoid cross-entropy tail of ONE task on one 1024-thread workgroup, shared by sigmoid_ce_kernel (csrc/tail.hip) and
// multitask_sigmoid_ce_kernel (csrc/mmoe.hip) so that a task's loss, probabilities and gradient are the same bits in both.
#pragma once
#include "common.h"

// store_prob(i, p), store_dlogit(i, d * grad_scale / B) (the latter only when want_dlogit).  red: 16 floats of LDS.
// -> the mean loss, valid in thread 0.  The caller synchronises before `red` is used again.
template <typename StoreProb, typename StoreDlogit>
__device__ __forceinline__ float sigmoid_ce_task(const float* __restrict__ logits, const float* __restrict__ labels,
                                                 unsigned B, float grad_scale, bool want_dlogit, float* red,
                                                 StoreProb store_prob, StoreDlogit store_dlogit) {
    float acc = 0.f;
    const float invB = 1.0f / (float)B;
    for (unsigned i = threadIdx.x; i < B; i += 1024) {
        float x = logits[i], z = labels[i];
        float ax = fabsf(x);
        float e = expf(-ax);
        // tf.nn.sigmoid_cross_entropy_with_logits: max(x,0) - x*z + log1p(exp(-|x|))
        acc += fmaxf(x, 0.f) - x * z + log1pf(e);
        float r = e / (1.0f + e);
        float p = x >= 0.f ? 1.0f / (1.0f + e) : r;
        store_prob(i, p);
        // d/dx in the form TF's autodiff of the three terms produces:
        //   [x>=0] - z -/+ e/(1+e)     (keeps 1e-13-size gradients at |x| ~ 30)
        if (want_dlogit) {
            float d = ((x >= 0.f ? 1.0f : 0.f) - z) + (x >= 0.f ? -r : r);
            store_dlogit(i, d * grad_scale * invB);
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    float v = 0.f;
    if (threadIdx.x < 64) {
        v = threadIdx.x < 16 ? red[threadIdx.x] : 0.f;
        v = wave_sum(v);
    }
    return v * invB;
}
