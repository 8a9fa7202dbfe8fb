// The fixed-order sums of every two-pass backward (weight-gradient split slabs, partial rows): the job descriptor and the three
// summation bodies.  Two kernels run them — dense_sum_slabs_kernel (dense.hip: the sums alone) and sums_adam_tf1_step_kernel
// (tail.hip: the sums and the dense optimizer update of the summed words in one launch) — and must agree bit for bit, so the
// order and the association of every sum are stated here, once.  The entries of bst.hip, dien.hip and din.hip that sum their own
// partial rows (the immediate second pass) run the same body: recalgo_slabs::launch_colsums below, a thin kernel around sum_tall.
// Two older copies of sum_tall's order remain — colsum16_kernel (common.h: mlp, tail, fibinet) and colsum4_kernel (cross.hip):
// through launch_colsums those entries measured 0.5-0.9 us slower per launch, and the cause is not found yet (DESIGN.md "One
// second pass").  tests/test_gpu_colsums.py holds cross.hip's copy to the same bits.
#pragma once
#include "common.h"

namespace recalgo_slabs {

constexpr int kMaxSplitJobs = 32;
struct SplitJob {
    const float* partials;
    float* out0;
    float* out1;
    unsigned long long slab, n0, n;
    int S, vec;                // vec: 1 float4 per thread, 0 one float per thread, 2 "tall" (S >> n): 16 columns x 16 row
                               //      groups per workgroup (a thread walking hundreds of partial rows alone is latency bound)
    unsigned first_block;      // blocks [first_block, next job's first_block) belong to this job
};

// where element i of a job's [0, n) goes: [0, n0) -> out0 (dW), [n0, n) -> out1 (dbias)
__device__ __forceinline__ float* job_target(const SplitJob& jb, size_t i) {
    return i < jb.n0 ? jb.out0 + i : jb.out1 + (i - jb.n0);
}

// vec == 1: elements [i, i + 4) of every slab, i % 4 == 0, i < jb.n, added in slab order (the sum's order is fixed).  The slab
// loads are independent: eight in flight per thread, the last round's surplus switched off (S is uniform).  A thread that
// takes a round trip per slab, as the tail of a four-wide loop did, spends 4 round trips on 8 slabs and 10 on 32.
__device__ __forceinline__ float4 sum_slabs4(const SplitJob& jb, size_t i) {
    const float* base = jb.partials + i;
    float4 acc = *reinterpret_cast<const float4*>(base);
    for (int s = 1; s < jb.S; s += 8) {
        float4 a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (s + u < jb.S) a[u] = *reinterpret_cast<const float4*>(base + (size_t)(s + u) * jb.slab);
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (s + u < jb.S) acc = f4_add(acc, a[u]);
    }
    return acc;
}

// vec == 0: element t < jb.n of every slab, in slab order
__device__ __forceinline__ float sum_slabs1(const SplitJob& jb, size_t t) {
    float acc = jb.partials[t];
    for (int s = 1; s < jb.S; ++s) acc += jb.partials[(size_t)s * jb.slab + t];
    return acc;
}

// vec == 2: ALL 256 threads of the workgroup (a barrier inside); tile: the workgroup's number within its job; sh: 16 x 17 floats
// of LDS.  Thread (rg, cl) = (threadIdx.x >> 4, threadIdx.x & 15) adds the partial rows rg, rg + 16, .. of column c = tile * 16 + cl
// in row order — they are independent loads: sixteen in flight per thread, the rows past the end switched off (a loop of
// load -> wait -> add over the 512 partial rows of the loss tail was most of the sum launch: ~13 us in the step) — then the
// threads with rg == 0 add the 16 group sums in group order: they return the column's sum (c < jb.n), every other thread 0.
__device__ __forceinline__ float sum_tall(const SplitJob& jb, size_t tile, float (*sh)[17]) {
    const unsigned cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const size_t c = tile * 16 + cl;
    float acc = 0.f;
    if (c < jb.n) {
        const float* col = jb.partials + c;
        for (int r = rg; r < jb.S; r += 16 * 16) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (r + 16 * u < jb.S) v[u] = col[(size_t)(r + 16 * u) * jb.slab];
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (r + 16 * u < jb.S) acc += v[u];
        }
    }
    sh[rg][cl] = acc;
    __syncthreads();
    float tt = 0.f;
    if (rg == 0 && c < jb.n) {
#pragma unroll
        for (int g = 0; g < 16; ++g) tt += sh[g][cl];
    }
    return tt;
}

}  // namespace recalgo_slabs

// The host side of the job table (dense.hip owns the split counts and the slab layout): the jobs of
// recalgo_dense_bwd_weights_reduce's two arrays, column sums first, in the block layout of dense_sum_slabs_kernel.
// -> 0, hipErrorInvalidValue for a bad descriptor, or -1 when more than `cap` jobs would be needed.
int recalgo_build_split_jobs(const recalgo_dense_split_t* jobs, int n_jobs, const recalgo_colsum_t* sums, int n_sums,
                             recalgo_slabs::SplitJob* out, int cap, int* n_out, unsigned* blocks);

namespace recalgo_slabs {

constexpr int kMaxColsumOuts = 8;

// An entry's immediate second pass.  The entry's partial rows are `count` (1..kMaxColsumOuts) gradients
// side by side: columns [starts[s], starts[s + 1]) of every row belong to outs[s]; starts[0] == 0, every run is non-empty and
// starts[count] is the row's length (the rows are contiguous).  outs[s][i] = the sum_tall sum of column starts[s] + i over the
// `rows` rows: the bits a recalgo_colsum_t job {partials + starts[s], outs[s], rows, starts[count], the run's length} of the
// step's deferred launch gives.  One launch (dense.hip: colsum_rows_kernel).
// -> the launch's hipError_t (it also reports a failed launch of the kernel that wrote the rows), or hipErrorInvalidValue.
int launch_colsums(const float* partials, int rows, int count, float* const* outs, const int* starts, hipStream_t st);

}  // namespace recalgo_slabs
