// The per-group AUC of an evaluation (include/recalgo_gauc.h): uAUC / GAUC as integer pair counts per group.
//   append   one launch per batch: row i of the batch goes to log position cursor + i (group id as int32, -1 for a row without a
//            group; one prediction per task; the tasks' label bits in one byte).  The cursor is a device word: every workgroup
//            reads it, the last one to finish (arrival ticket, the idiom of tail.hip's adam_publish_step) advances it, so a
//            captured launch appends behind its previous replay.  A latency chain like metrics.hip (4096 rows: 16 workgroups).
//   finish   count rows per group -> exclusive scan over the groups (256-wide tiles, three launches: tile sums, the scan of the
//            tile sums by one workgroup, the tiles again) -> place the rows by group -> pair counts.
//   * the two kernels that add into a per-group word (count, place) first match the lanes of a wave that hold the same group
//     (wave_match: ballots only), so one group holding every row costs one atomic per wave, not one per row;
//   * the pair kernel gives every placed row a thread: a workgroup owns 256 consecutive positions of the grouped log and stages
//     the union of their groups' ranges through LDS in tiles of 1024 rows — only the tile's positive rows, compacted by a block
//     scan, with the number of positive rows before each row of the tile, so that a group's part of a tile is a range of the
//     compacted list.  Each NEGATIVE row walks the positive rows of its own group: with the few positives of click data the
//     walk is short and nearly every lane takes part (a group of mostly positive rows costs a walk as long as its positives).
//     One group's pair work is so spread over its rows; the sums of a wave's runs of equal groups are added by the run's first
//     lane (segmented shuffle);
//   * integer additions only (32-bit and 64-bit vector atomics from C++), so every count is the same in whatever order the
//     workgroups arrive.
#include <algorithm>

#include "common.h"
#include "plan_scan.h"
#include "../../include/recalgo_gauc.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxTasks = RECALGO_GAUC_MAX_TASKS;
constexpr int kHeaderWords = RECALGO_GAUC_STATE_HEADER_WORDS;
constexpr int kResultHeader = RECALGO_GAUC_RESULT_HEADER_WORDS;
constexpr int kPairTile = 1024;                          // grouped rows of one LDS tile of the pair kernel
constexpr int kSweepBlocks = 2048;                       // workgroups of a sweep over the log (grid-stride)
constexpr int kPairBlocks = 16384;

__host__ __device__ inline long long pad_to(long long v, long long m) { return (v + m - 1) / m * m; }

// the row log (in the state buffer behind its header, and once more in the workspace, in group order)
struct Log {
    int* group;               // [Cp]
    float* prediction;        // [T][Cp]
    unsigned char* labels;    // [Cp]
    long long Cp;
};
inline long long log_bytes(int T, int C) { return pad_to(C, 4) * (5 + 4ll * T); }
inline Log log_at(void* base, int T, int C) {
    Log L;
    L.Cp = pad_to(C, 4);
    L.group = static_cast<int*>(base);
    L.prediction = reinterpret_cast<float*>(L.group + L.Cp);
    L.labels = reinterpret_cast<unsigned char*>(L.prediction + (long long)T * L.Cp);
    return L;
}
inline bool shape_ok(int G, int T, int C) {
    return T >= 1 && T <= kMaxTasks && G >= 1 && G <= RECALGO_GAUC_MAX_GROUPS && C >= 1 && C <= RECALGO_GAUC_MAX_ROWS;
}

// the finish's scratch
struct Work {
    unsigned* count;          // [Gp]   rows of group g
    unsigned* first;          // [Gp]   first grouped position of group g
    unsigned* fill;           // [Gp]   next free grouped position of group g
    unsigned* tile_sum;       // [nbp + 256]   the 256-wide tiles' sums, then their exclusive scan; word nbp: rows with a group
    Log sorted;
    int nb, nbp;
};
inline long long work_bytes(int G, int T, int C) {
    const long long Gp = pad_to(G, 256), nbp = pad_to(Gp / 256, 256);
    return pad_to(4 * (3 * Gp + nbp + 256) + log_bytes(T, C), 8);
}
inline Work work_at(void* base, int G, int T, int C) {
    const long long Gp = pad_to(G, 256);
    Work W;
    W.nb = (int)(Gp / 256);
    W.nbp = (int)pad_to(W.nb, 256);
    W.count = static_cast<unsigned*>(base);
    W.first = W.count + Gp;
    W.fill = W.first + Gp;
    W.tile_sum = W.fill + Gp;
    W.sorted = log_at(W.tile_sum + W.nbp + 256, T, C);
    return W;
}

// ---- append -------------------------------------------------------------------------------------------------------------
struct Column {
    const float* labels;
    const float* predictions;
    int label_step, prediction_step;
};
struct AppendArgs {
    Column col[kMaxTasks];
    const long long* groups;
    unsigned long long* header;
    Log log;
    int group_step, T, n, G, C;
};

__global__ __launch_bounds__(kThreads) void gauc_append_kernel(AppendArgs A) {
    __shared__ unsigned long long s_cursor;
    if (threadIdx.x == 0) s_cursor = __hip_atomic_load(&A.header[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const unsigned long long cursor = s_cursor;
    const int i = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (i < A.n && cursor + (unsigned long long)i < (unsigned long long)A.C) {
        const long long k = (long long)cursor + i;
        const long long g = A.groups[(size_t)i * A.group_step];
        A.log.group[k] = (g >= 0 && g < A.G) ? (int)g : -1;
        unsigned bits = 0;
        for (int t = 0; t < A.T; ++t) {
            const Column& c = A.col[t];
            A.log.prediction[t * A.log.Cp + k] = c.predictions[(size_t)i * c.prediction_step];
            bits |= (c.labels[(size_t)i * c.label_step] > 0.5f ? 1u : 0u) << t;
        }
        A.log.labels[k] = (unsigned char)bits;
    }
    // every workgroup has read the cursor (its value went through LDS above) before it draws its ticket, so the last arrival may
    // overwrite it; the stores are drained and released before the ticket, in the order of the split-K reducer's hand-off
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long arrived = __hip_atomic_fetch_add(&A.header[2], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (arrived == (unsigned long long)gridDim.x - 1ull) {
            __hip_atomic_store(&A.header[2], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long end = cursor + (unsigned long long)A.n, C = (unsigned long long)A.C;
            const unsigned long long over = end > C ? end - C : 0ull;                 // positions >= C among [cursor, end)
            A.header[1] = A.header[1] + (over < (unsigned long long)A.n ? over : (unsigned long long)A.n);
            A.header[0] = end;
        }
    }
}

// ---- finish -------------------------------------------------------------------------------------------------------------
// The lanes of a wave that hold the same group: `leader` the lowest of them, `cnt` how many, `rank` this lane's place among
// them.  Ballots only; all 64 lanes call it (a lane without a group passes valid = false and gets cnt 0).
__device__ __forceinline__ void wave_match(int g, bool valid, int& leader, unsigned& cnt, unsigned& rank) {
    const int lane = (int)(threadIdx.x & 63);
    unsigned long long todo = __ballot(valid);
    leader = lane, cnt = 0u, rank = 0u;
    while (todo) {                                       // (wave-uniform)
        const int l = __ffsll((long long)todo) - 1;
        const int lg = __shfl(g, l, 64);
        const bool mine = valid && g == lg;
        const unsigned long long m = __ballot(mine);
        if (mine) {
            leader = l;
            cnt = (unsigned)__popcll(m);
            rank = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        }
        todo &= ~m;
    }
}

struct FinishArgs {
    const unsigned long long* header;
    Log log;
    Work work;
    unsigned long long* result;
    int G, T, C;
};

__device__ __forceinline__ long long logged_rows(const FinishArgs& F) {
    const unsigned long long cursor = F.header[0];
    return (long long)(cursor < (unsigned long long)F.C ? cursor : (unsigned long long)F.C);
}

__global__ __launch_bounds__(kThreads) void gauc_count_kernel(FinishArgs F) {
    const long long rows = logged_rows(F);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        F.result[1] = F.header[1];
        F.result[2] = (unsigned long long)rows;
    }
    unsigned skipped = 0;
    for (long long base = (long long)blockIdx.x * kThreads; base < rows; base += (long long)gridDim.x * kThreads) {
        const long long i = base + threadIdx.x;
        const int g = i < rows ? F.log.group[i] : -1;
        skipped += (i < rows && g < 0) ? 1u : 0u;
        int leader;
        unsigned cnt, rank;
        wave_match(g, g >= 0, leader, cnt, rank);
        if (g >= 0 && rank == 0u) atomicAdd(&F.work.count[g], cnt);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) skipped += __shfl_xor(skipped, o, 64);
    if ((threadIdx.x & 63) == 0 && skipped) atomicAdd(&F.result[0], (unsigned long long)skipped);
}

// count[] in 256-wide tiles (the padding behind G is zero): a tile's sum
__global__ __launch_bounds__(kThreads) void gauc_scan_tiles_kernel(Work W) {
    __shared__ unsigned sh[8];
    unsigned total;
    recalgo_plan::excl_scan256(W.count[(size_t)blockIdx.x * 256 + threadIdx.x], sh, total);
    if (threadIdx.x == 0) W.tile_sum[blockIdx.x] = total;
}
// one workgroup: the tile sums become their exclusive scan, 256 at a time with a running carry
__global__ __launch_bounds__(kThreads) void gauc_scan_top_kernel(Work W) {
    __shared__ unsigned sh[8];
    unsigned carry = 0;
    for (int c = 0; c < W.nbp; c += 256) {
        const int b = c + (int)threadIdx.x;
        unsigned total;
        const unsigned e = recalgo_plan::excl_scan256(b < W.nb ? W.tile_sum[b] : 0u, sh, total);
        if (b < W.nb) W.tile_sum[b] = carry + e;
        carry += total;
    }
    if (threadIdx.x == 0) W.tile_sum[W.nbp] = carry;
}
__global__ __launch_bounds__(kThreads) void gauc_scan_apply_kernel(Work W) {
    __shared__ unsigned sh[8];
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned total;
    const unsigned e = recalgo_plan::excl_scan256(W.count[g], sh, total) + W.tile_sum[blockIdx.x];
    W.first[g] = e;
    W.fill[g] = e;
}

__global__ __launch_bounds__(kThreads) void gauc_place_kernel(FinishArgs F) {
    const long long rows = logged_rows(F);
    for (long long base = (long long)blockIdx.x * kThreads; base < rows; base += (long long)gridDim.x * kThreads) {
        const long long i = base + threadIdx.x;
        const int g = i < rows ? F.log.group[i] : -1;
        int leader;
        unsigned cnt, rank;
        wave_match(g, g >= 0, leader, cnt, rank);
        unsigned at = 0;
        if (g >= 0 && rank == 0u) at = atomicAdd(&F.work.fill[g], cnt);
        at = __shfl(at, leader, 64) + rank;
        if (g >= 0) {
            F.work.sorted.group[at] = g;
            F.work.sorted.labels[at] = F.log.labels[i];
            for (int t = 0; t < F.T; ++t) F.work.sorted.prediction[t * F.log.Cp + at] = F.log.prediction[t * F.log.Cp + i];
        }
    }
}

__global__ __launch_bounds__(kThreads) void gauc_pairs_kernel(FinishArgs F) {
    __shared__ float tile[kPairTile];                    // the predictions of the tile's positive rows, one behind the other
    __shared__ unsigned before[kPairTile + 1];           // positive rows among the tile's rows [0, k)
    __shared__ unsigned span[2];
    __shared__ unsigned scan_sh[8];
    static_assert(kPairTile == 4 * kThreads, "a thread stages four consecutive rows of a tile");
    const Work& W = F.work;
    const int t = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63;
    const long long placed = (long long)W.tile_sum[W.nbp];
    const float* const pred = W.sorted.prediction + t * W.sorted.Cp;
    for (long long s0 = (long long)blockIdx.x * kThreads; s0 < placed; s0 += (long long)gridDim.x * kThreads) {
        const long long s = s0 + tid;
        const bool active = s < placed;
        const int g = active ? W.sorted.group[s] : -1;
        const unsigned lo = active ? W.first[g] : 0u, hi = active ? lo + W.count[g] : 0u;
        const bool y = active && ((W.sorted.labels[s] >> t) & 1u);
        const float q = active ? pred[s] : 0.f;
        // groups lie in the grouped log in ascending order: the union of this workgroup's ranges is first row's lo .. last row's hi
        if (tid == 0) span[0] = lo;
        if (s == placed - 1 || (active && tid == kThreads - 1)) span[1] = hi;
        __syncthreads();
        const unsigned ulo = span[0], uhi = span[1];
        unsigned acc = 0;                                 // <= 2 C < 2^30
        for (unsigned b = ulo; b < uhi; b += kPairTile) {
            const unsigned len = min((unsigned)kPairTile, uhi - b);
            // stage: the tile's positive rows compacted, and for every row of the tile how many positive rows lie before it
            float v[4];
            bool yy[4];
            unsigned mine = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned k = 4u * tid + i;
                yy[i] = k < len && ((W.sorted.labels[b + k] >> t) & 1u);
                v[i] = yy[i] ? pred[b + k] : 0.f;
                mine += yy[i] ? 1u : 0u;
            }
            unsigned total;
            unsigned at = recalgo_plan::excl_scan256(mine, scan_sh, total);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                before[4 * tid + i] = at;
                if (yy[i]) tile[at++] = v[i];
            }
            if (tid == kThreads - 1) before[kPairTile] = total;
            __syncthreads();
            // a negative row meets the positive rows of its own group that this tile holds
            const unsigned from = max(lo, b), to = min(hi, b + len);
            if (active && !y && from < to) {
                const unsigned end = before[to - b];
                for (unsigned j = before[from - b]; j < end; ++j) {
                    const float p = tile[j];
                    acc += p > q ? 2u : (p == q ? 1u : 0u);
                }
            }
            __syncthreads();
        }
        // a wave's runs of equal groups: the run's first lane ends up with the run's sums
        unsigned long long sum = acc;
        unsigned pn = active ? (y ? 1u : 1u << 16) : 0u;    // positives | negatives << 16
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long sum2 = __shfl_down(sum, o, 64);
            const unsigned pn2 = __shfl_down(pn, o, 64);
            const int g2 = __shfl_down(g, o, 64);
            if (lane + o < 64 && g2 == g) sum += sum2, pn += pn2;
        }
        const int before = __shfl_up(g, 1, 64);
        if (active && (lane == 0 || before != g)) {
            unsigned long long* const num2 = F.result + kResultHeader + ((size_t)t * F.G + g);
            const size_t TG = (size_t)F.T * F.G;
            if (sum) atomicAdd(num2, sum);
            if (pn & 0xffffu) atomicAdd(num2 + TG, (unsigned long long)(pn & 0xffffu));
            if (pn >> 16) atomicAdd(num2 + 2 * TG, (unsigned long long)(pn >> 16));
        }
    }
}

}  // namespace

RECALGO_EXPORT int recalgo_gauc_abi_version(void) { return RECALGO_GAUC_ABI_VERSION; }

RECALGO_EXPORT int64_t recalgo_gauc_state_bytes(int G, int T, int C) {
    if (!shape_ok(G, T, C)) return 0;
    return (int64_t)pad_to(8ll * kHeaderWords + log_bytes(T, C), 8);
}

RECALGO_EXPORT int64_t recalgo_gauc_workspace_bytes(int G, int T, int C) {
    if (!shape_ok(G, T, C)) return 0;
    return (int64_t)work_bytes(G, T, C);
}

RECALGO_EXPORT int recalgo_gauc_append(const int64_t* groups, int group_step, const recalgo_gauc_column_t* columns, int T, int n,
                                       int G, int C, void* state, recalgo_stream_t stream) {
    RECALGO_REQUIRE(n >= 1 && shape_ok(G, T, C) && groups && columns && state && group_step >= 1);
    RECALGO_REQUIRE(aligned_to<8>(groups) && aligned_to<8>(state));
    AppendArgs A = {};
    for (int t = 0; t < T; ++t) {
        const recalgo_gauc_column_t& in = columns[t];
        RECALGO_REQUIRE(in.labels && in.predictions && in.label_step >= 1 && in.prediction_step >= 1);
        RECALGO_REQUIRE(aligned_to<4>(in.labels) && aligned_to<4>(in.predictions));
        A.col[t] = Column{in.labels, in.predictions, in.label_step, in.prediction_step};
    }
    A.groups = reinterpret_cast<const long long*>(groups);
    A.header = static_cast<unsigned long long*>(state);
    A.log = log_at(A.header + kHeaderWords, T, C);
    A.group_step = group_step, A.T = T, A.n = n, A.G = G, A.C = C;
    hipLaunchKernelGGL(gauc_append_kernel, dim3(cdiv(n, kThreads)), dim3(kThreads), 0, as_stream(stream), A);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_gauc_finish(const void* state, int G, int T, int C, int64_t* result, void* workspace,
                                       recalgo_stream_t stream) {
    RECALGO_REQUIRE(shape_ok(G, T, C) && state && result && workspace);
    RECALGO_REQUIRE(aligned_to<8>(state) && aligned_to<8>(result) && aligned_to<8>(workspace));
    hipStream_t st = as_stream(stream);
    FinishArgs F = {};
    F.header = static_cast<const unsigned long long*>(state);
    F.log = log_at(const_cast<unsigned long long*>(F.header) + kHeaderWords, T, C);
    F.work = work_at(workspace, G, T, C);
    F.result = reinterpret_cast<unsigned long long*>(result);
    F.G = G, F.T = T, F.C = C;
    const Work& W = F.work;
    RECALGO_CHECK(hipMemsetAsync(result, 0, 8 * ((size_t)kResultHeader + 3 * (size_t)T * G), st));
    RECALGO_CHECK(hipMemsetAsync(W.count, 0, 4 * (size_t)W.nb * 256, st));
    const int sweep = std::min(cdiv(C, kThreads), kSweepBlocks);
    hipLaunchKernelGGL(gauc_count_kernel, dim3(sweep), dim3(kThreads), 0, st, F);
    hipLaunchKernelGGL(gauc_scan_tiles_kernel, dim3(W.nb), dim3(kThreads), 0, st, W);
    hipLaunchKernelGGL(gauc_scan_top_kernel, dim3(1), dim3(kThreads), 0, st, W);
    hipLaunchKernelGGL(gauc_scan_apply_kernel, dim3(W.nb), dim3(kThreads), 0, st, W);
    hipLaunchKernelGGL(gauc_place_kernel, dim3(sweep), dim3(kThreads), 0, st, F);
    hipLaunchKernelGGL(gauc_pairs_kernel, dim3(std::min(cdiv(C, kThreads), kPairBlocks), T), dim3(kThreads), 0, st, F);
    RECALGO_RETURN_LAST();
}
