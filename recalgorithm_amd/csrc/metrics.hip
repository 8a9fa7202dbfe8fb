// The streaming metrics of one EVAL batch in ONE launch (include/recalgo_metrics.h, and over the rows a mask selects
// include/recalgo_maskmetrics.h: one kernel body, MASKED or not): per slot an AUC histogram
//     hist[label > 0.5][#{j : p > th[j]}] += 1
// or an accuracy count, plus the loss accumulator.  The host turns the histograms into tp / fp / fn / tn once, at the end of the
// evaluation; per batch nothing comes back.  A latency chain, not a throughput kernel (4096 rows x 6 slots: 24 workgroups):
//   * grid (row chunks, slots); a workgroup owns kRows consecutive rows of one slot;
//   * AUC: the thresholds and a zeroed 2 x (N + 1) histogram in LDS, one binary search per row over the LDS copy (the predicate
//     p > th[j] is monotone in j for an ascending array, false everywhere for a NaN), one 32-bit LDS atomic per row, then one
//     64-bit global atomic per non-empty bin;
//   * accuracy: a sum over each wave, one LDS atomic per wave, one global atomic per workgroup;
//   * integer additions only, so the counts are the same bits in whatever order the workgroups arrive; plain vector stores and
//     atomics from C++; the loss is added by one thread of one workgroup (launches on a stream are ordered);
//   * MASKED: a row takes part iff its slot has no mask or mask[i] > 0.5 (false for a NaN); a row that does not is skipped before
//     anything is read of it, and an accuracy slot counts the rows that take part (one more wave sum) instead of adding n.
//     The unmasked instantiation reads no mask field: its launches, grid and counts are those of before the mask existed.
#include "common.h"
#include "../../include/recalgo_metrics.h"
#include "../../include/recalgo_maskmetrics.h"

static_assert(RECALGO_MASKMETRICS_MAX_SLOTS == RECALGO_METRICS_MAX_SLOTS && RECALGO_MASKMETRICS_MAX_THRESHOLDS == RECALGO_METRICS_MAX_THRESHOLDS &&
                  RECALGO_MASKMETRICS_AUC == RECALGO_METRICS_AUC && RECALGO_MASKMETRICS_ACCURACY == RECALGO_METRICS_ACCURACY,
              "the two headers share one kernel body and one state layout");

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 1024;                               // rows of one workgroup
constexpr int kMaxSlots = RECALGO_METRICS_MAX_SLOTS;
constexpr int kMaxN = RECALGO_METRICS_MAX_THRESHOLDS;

struct Slot {
    const float* labels;
    const float* predictions;
    const float* thresholds;
    int kind, N, label_stride, prediction_stride;
    long long first_word;                                 // of the slot's counters in the state buffer
    const float* mask;                                    // MASKED only; nullptr: every row takes part
    int mask_step;
};
struct MetricsArgs {
    Slot slot[kMaxSlots];
    const float* loss;
    unsigned long long* state;
    int n;
};

template <bool MASKED>
__global__ __launch_bounds__(kThreads) void metrics_update_kernel(MetricsArgs P) {
    __shared__ float th[kMaxN];
    __shared__ unsigned hist[2 * (kMaxN + 1)];
    const Slot& S = P.slot[blockIdx.y];
    const int tid = (int)threadIdx.x;
    const int r0 = (int)blockIdx.x * kRows;
    const int rows = min(kRows, P.n - r0);                // (r0 < n: the grid is cdiv(n, kRows) chunks)
    unsigned long long* const out = P.state + S.first_word;
    const float* const mask = MASKED ? S.mask : nullptr;
    auto takes_part = [&](size_t i) { return !MASKED || mask == nullptr || mask[i * S.mask_step] > 0.5f; };

    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0 && P.loss != nullptr) {
        double* const sum = reinterpret_cast<double*>(P.state);
        *sum = *sum + (double)*P.loss;
        P.state[1] = P.state[1] + 1ull;
    }

    if (S.kind == RECALGO_METRICS_ACCURACY) {
        if (tid == 0) hist[0] = hist[1] = 0u;
        __syncthreads();
        unsigned mine = 0, part = 0;                      // part: the rows of a masked slot that take part
        for (int k = tid; k < rows; k += kThreads) {
            const size_t i = (size_t)(r0 + k);
            if (!takes_part(i)) continue;
            mine += S.labels[i * S.label_stride] == S.predictions[i * S.prediction_stride] ? 1u : 0u;
            part += 1u;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
        if ((tid & 63) == 0 && mine) atomicAdd(&hist[0], mine);
        if (MASKED && mask != nullptr) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
            if ((tid & 63) == 0 && part) atomicAdd(&hist[1], part);
        }
        __syncthreads();
        if (tid == 0) {
            if (hist[0]) atomicAdd(&out[0], (unsigned long long)hist[0]);
            if (MASKED && mask != nullptr) {
                if (hist[1]) atomicAdd(&out[1], (unsigned long long)hist[1]);
            } else if (blockIdx.x == 0) {
                atomicAdd(&out[1], (unsigned long long)P.n);
            }
        }
        return;
    }

    const int N = S.N, bins = 2 * (N + 1);
    for (int j = tid; j < N; j += kThreads) th[j] = S.thresholds[j];
    for (int b = tid; b < bins; b += kThreads) hist[b] = 0u;
    __syncthreads();
    for (int k = tid; k < rows; k += kThreads) {
        const size_t i = (size_t)(r0 + k);
        if (!takes_part(i)) continue;
        const float p = S.predictions[i * S.prediction_stride];
        const int y = S.labels[i * S.label_stride] > 0.5f ? 1 : 0;
        int lo = 0, hi = N;                               // th[j] < p for j < lo, !(p > th[j]) for j >= hi
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (p > th[mid]) lo = mid + 1;
            else hi = mid;
        }
        atomicAdd(&hist[y * (N + 1) + lo], 1u);
    }
    __syncthreads();
    for (int b = tid; b < bins; b += kThreads) {
        const unsigned c = hist[b];
        if (c) atomicAdd(&out[b], (unsigned long long)c);
    }
}

// words of a slot's counters; 0: a slot the kernel does not serve
long long slot_words(int kind, int num_thresholds) {
    if (kind == RECALGO_METRICS_ACCURACY) return 2;
    if (kind != RECALGO_METRICS_AUC || num_thresholds < 2 || num_thresholds > kMaxN) return 0;
    return 2ll * (num_thresholds + 1);
}

template <typename SlotIn>
int64_t state_bytes(const SlotIn* slots, int n_slots) {
    if (!slots || n_slots < 1 || n_slots > kMaxSlots) return 0;
    long long words = 2;
    for (int s = 0; s < n_slots; ++s) {
        const long long w = slot_words(slots[s].kind, slots[s].num_thresholds);
        if (!w) return 0;
        words += w;
    }
    return (int64_t)(words * 8);
}

// the two headers' slots, field by field
const float* mask_of(const recalgo_metrics_slot_t&) { return nullptr; }
const float* mask_of(const recalgo_maskmetrics_slot_t& s) { return s.mask; }
int mask_step_of(const recalgo_metrics_slot_t&) { return 1; }
int mask_step_of(const recalgo_maskmetrics_slot_t& s) { return s.mask_step; }
int label_step_of(const recalgo_metrics_slot_t& s) { return s.label_stride; }
int label_step_of(const recalgo_maskmetrics_slot_t& s) { return s.label_step; }
int prediction_step_of(const recalgo_metrics_slot_t& s) { return s.prediction_stride; }
int prediction_step_of(const recalgo_maskmetrics_slot_t& s) { return s.prediction_step; }

template <bool MASKED, typename SlotIn>
int update(const SlotIn* slots, int n_slots, const float* loss, int n, void* state, recalgo_stream_t stream) {
    RECALGO_REQUIRE(n >= 1 && slots && state && n_slots >= 1 && n_slots <= kMaxSlots);
    RECALGO_REQUIRE(aligned_to<8>(state) && aligned_to<4>(loss));
    MetricsArgs P = {};
    long long word = 2;
    for (int s = 0; s < n_slots; ++s) {
        const SlotIn& in = slots[s];
        const long long w = slot_words(in.kind, in.num_thresholds);
        RECALGO_REQUIRE(w && in.labels && in.predictions && label_step_of(in) >= 1 && prediction_step_of(in) >= 1);
        RECALGO_REQUIRE(aligned_to<4>(in.labels) && aligned_to<4>(in.predictions));
        const bool auc = in.kind == RECALGO_METRICS_AUC;
        RECALGO_REQUIRE(!auc || (in.thresholds && aligned_to<4>(in.thresholds)));
        const float* const mask = mask_of(in);
        RECALGO_REQUIRE(mask == nullptr || (mask_step_of(in) >= 1 && aligned_to<4>(mask)));
        Slot& S = P.slot[s];
        S.labels = in.labels;
        S.predictions = in.predictions;
        S.thresholds = auc ? in.thresholds : nullptr;
        S.kind = in.kind;
        S.N = auc ? in.num_thresholds : 0;
        S.label_stride = label_step_of(in);
        S.prediction_stride = prediction_step_of(in);
        S.first_word = word;
        S.mask = mask;
        S.mask_step = mask ? mask_step_of(in) : 1;
        word += w;
    }
    P.loss = loss;
    P.state = static_cast<unsigned long long*>(state);
    P.n = n;
    hipLaunchKernelGGL(metrics_update_kernel<MASKED>, dim3(cdiv(n, kRows), n_slots), dim3(kThreads), 0, as_stream(stream), P);
    RECALGO_RETURN_LAST();
}

}  // namespace

RECALGO_EXPORT int recalgo_metrics_abi_version(void) { return RECALGO_METRICS_ABI_VERSION; }
RECALGO_EXPORT int recalgo_maskmetrics_abi_version(void) { return RECALGO_MASKMETRICS_ABI_VERSION; }

RECALGO_EXPORT int64_t recalgo_metrics_state_bytes(const recalgo_metrics_slot_t* slots, int n_slots) {
    return state_bytes(slots, n_slots);
}
RECALGO_EXPORT int64_t recalgo_maskmetrics_state_bytes(const recalgo_maskmetrics_slot_t* slots, int n_slots) {
    return state_bytes(slots, n_slots);
}

RECALGO_EXPORT int recalgo_metrics_update(const recalgo_metrics_slot_t* slots, int n_slots, const float* loss, int n, void* state,
                                          recalgo_stream_t stream) {
    return update<false>(slots, n_slots, loss, n, state, stream);
}
RECALGO_EXPORT int recalgo_maskmetrics_update(const recalgo_maskmetrics_slot_t* slots, int n_slots, const float* loss, int n,
                                              void* state, recalgo_stream_t stream) {
    return update<true>(slots, n_slots, loss, n, state, stream);
}
