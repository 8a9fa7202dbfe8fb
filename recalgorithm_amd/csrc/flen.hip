// FLEN's field-wise bi-interaction with Dicefactor (include/recalgo_flen.h; Chen et al., arXiv 1911.04690), one kernel each way.
//
// All of the arithmetic is element-wise in the embedding component k, so a group of KV = K / 4 lanes serves an example, each
// lane a float4 of components, and nothing crosses lanes but the weight gradients.  A workgroup is one wave: T = floor(64 / KV)
// examples at a time (for KV = 3, 5, 6, .. the last 64 - T KV lanes idle), workgroup s walking the tiles s, s + grid, ..  A lane
// keeps e_m and q_m of its example in registers (2 M float4, M a template parameter so that every index is static) and reads
// each field row as one 16-byte piece: the host sorts the fields by group (ascending f inside a group, the header's order) and
// the kernels walk that list, so `group_of` never indexes a register array.  No LDS in the forward.
//
// The backward walks the rows twice (e and q, then dx).  A lane adds its examples' dr_mf, dr_fm and its four dbias components
// in registers, tile after tile; at the end the wave lays them out in LDS and sums them lane by lane in lane order — any KV,
// a power of two or not, is the same loop — into the workgroup's partial row.  recalgo_slabs::launch_colsums sums the rows.
//
// Dicefactor: c[path] comes from csrc/dropout.h's hash (or the explicit mask) at element (b (P + M) + path) K + k, in the
// forward and again in the backward; no mask is stored.
#include "common.h"
#include "dropout.h"
#include "slab_sum.h"
#include "../../include/recalgo_flen.h"

namespace {

constexpr int kLanes = RECALGO_FLEN_LANES;
constexpr int kMaxF = RECALGO_FLEN_MAX_F;
constexpr int kMaxM = RECALGO_FLEN_MAX_M;
constexpr int kMaxRows = RECALGO_FLEN_MAX_PARTIAL_ROWS;
constexpr int kMaxCols = kMaxM * (kMaxM - 1) / 2 + kMaxM + 4;      // a lane's sums: dr_mf, dr_fm, four dbias components
constexpr int kLd = kMaxCols + 1;                                  // (odd: the lanes' rows start on different banks)

// the fields sorted by group: order[start[m] .. start[m + 1]) are group m's, ascending
struct FlPlan {
    unsigned char order[kMaxF];
    unsigned char start[kMaxM + 1];
};

struct FlArgs {
    const float *x, *r_mf, *r_fm;
    int B, F, K;
    recalgo_drop::Spec dice;
    FlPlan plan;
};

bool shape_ok(int F, int M, int K) {
    return F >= RECALGO_FLEN_MIN_F && F <= RECALGO_FLEN_MAX_F && M >= RECALGO_FLEN_MIN_M && M <= RECALGO_FLEN_MAX_M && M <= F &&
           K >= RECALGO_FLEN_MIN_K && K <= RECALGO_FLEN_MAX_K && (K & 3) == 0;
}
int tile_of(int K) { return kLanes / (K >> 2); }
int workgroups(int B, int K) {
    const int tiles = cdiv(B, tile_of(K));
    return tiles > kMaxRows ? kMaxRows : tiles;
}

// group_of (host) -> the plan; false: an index outside [0, M) or an empty group
bool make_plan(const int32_t* group_of, int F, int M, FlPlan* plan) {
    int n = 0;
    for (int m = 0; m < M; ++m) {
        plan->start[m] = (unsigned char)n;
        for (int f = 0; f < F; ++f) {
            if (group_of[f] < 0 || group_of[f] >= M) return false;
            if (group_of[f] == m) plan->order[n++] = (unsigned char)f;
        }
        if (n == plan->start[m]) return false;
    }
    for (int m = M; m <= kMaxM; ++m) plan->start[m] = (unsigned char)n;
    for (int i = n; i < kMaxF; ++i) plan->order[i] = 0;
    return true;
}

// ---- device ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 f4_mul(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 f4_sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 f4_fma4(float4 a, float4 b, float4 c) {
    return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}
// e * e - q with the square ROUNDED first (no contraction into an fma): a group of one field has q = round(x * x) and gives 0
__device__ __forceinline__ float4 sq_minus(float4 e, float4 q) {
#pragma clang fp contract(off)
    const float sx = e.x * e.x, sy = e.y * e.y, sz = e.z * e.z, sw = e.w * e.w;
    return make_float4(sx - q.x, sy - q.y, sz - q.z, sw - q.w);
}

// the lane's place: which example of the tile, which four components
struct FlLane {
    int slot, k0;
    bool live;
};
__device__ __forceinline__ FlLane lane_of(int K) {
    const int kv = K >> 2, lane = threadIdx.x;
    FlLane l;
    l.slot = lane / kv;
    l.k0 = 4 * (lane - l.slot * kv);
    l.live = l.slot < kLanes / kv;
    return l;
}

// e_m and q_m of example b, components [k0, k0 + 4): one 16-byte read per field row
template <int M>
__device__ __forceinline__ void field_sums(const FlArgs& a, long long b, int k0, float4 (&e)[M], float4 (&q)[M]) {
    const float* xb = a.x + (size_t)b * a.F * a.K + k0;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        float4 em = f4_zero(), qm = f4_zero();
        for (int i = a.plan.start[m]; i < a.plan.start[m + 1]; ++i) {
            const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)a.plan.order[i] * a.K);
            em = f4_add(em, v), qm = f4_fma4(v, v, qm);
        }
        e[m] = em, q[m] = qm;
    }
}

// c[path] of example b (dice on), components [k0, k0 + 4)
__device__ __forceinline__ float4 dice4(const FlArgs& a, recalgo_drop::Key key, long long b, int paths, int path, int k0) {
    return recalgo_drop::factor4(a.dice, key, (uint32_t)(((unsigned long long)b * paths + path) * a.K + k0));
}

template <int M, bool DICED>
__global__ __launch_bounds__(kLanes) void flen_fwd_kernel(FlArgs a, const float* __restrict__ bias, float* __restrict__ e_out,
                                                          float* __restrict__ h_out) {
    constexpr int P = M * (M - 1) / 2;
    const FlLane l = lane_of(a.K);
    const int T = kLanes / (a.K >> 2), tiles = (a.B + T - 1) / T;
    constexpr bool diced = DICED;                            // (a template parameter: the plain path carries no hash state)
    recalgo_drop::Key key = {0u, 0u};
    if (diced) key = recalgo_drop::make_key(a.dice);
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long b = (long long)t * T + l.slot;
        if (!l.live || b >= a.B) continue;
        float4 e[M], q[M];
        field_sums<M>(a, b, l.k0, e, q);
        float4 h = *reinterpret_cast<const float4*>(bias + l.k0);
        int p = 0;
#pragma unroll
        for (int i = 0; i < M; ++i) {
#pragma unroll
            for (int j = i + 1; j < M; ++j, ++p) {
                float4 rc = f4_scale(make_float4(1.f, 1.f, 1.f, 1.f), a.r_mf[p]);
                if (diced) rc = f4_scale(dice4(a, key, b, P + M, p, l.k0), a.r_mf[p]);
                h = f4_fma4(rc, f4_mul(e[i], e[j]), h);
            }
        }
#pragma unroll
        for (int m = 0; m < M; ++m) {
            float4 rc = f4_scale(make_float4(1.f, 1.f, 1.f, 1.f), a.r_fm[m]);
            if (diced) rc = f4_scale(dice4(a, key, b, P + M, P + m, l.k0), a.r_fm[m]);
            h = f4_fma4(rc, sq_minus(e[m], q[m]), h);
            *reinterpret_cast<float4*>(e_out + ((size_t)b * M + m) * a.K + l.k0) = e[m];
        }
        *reinterpret_cast<float4*>(h_out + (size_t)b * a.K + l.k0) = h;
    }
}

template <int M, bool DICED>
__global__ __launch_bounds__(kLanes) void flen_bwd_kernel(FlArgs a, const float* __restrict__ g_e, const float* __restrict__ g_h,
                                                          float* __restrict__ dx, float* __restrict__ rows) {
    constexpr int P = M * (M - 1) / 2, C = P + M;
    __shared__ float sums[kLanes * kLd];
    const FlLane l = lane_of(a.K);
    const int kv = a.K >> 2, T = kLanes / kv, tiles = (a.B + T - 1) / T;
    constexpr bool diced = DICED;
    recalgo_drop::Key key = {0u, 0u};
    if (diced) key = recalgo_drop::make_key(a.dice);

    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    float4 db = f4_zero();
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long b = (long long)t * T + l.slot;
        if (!l.live || b >= a.B) continue;
        float4 e[M], q[M], tm[M];
        field_sums<M>(a, b, l.k0, e, q);
        const float4 gh = *reinterpret_cast<const float4*>(g_h + (size_t)b * a.K + l.k0);
        db = f4_add(db, gh);
#pragma unroll
        for (int m = 0; m < M; ++m) tm[m] = *reinterpret_cast<const float4*>(g_e + ((size_t)b * M + m) * a.K + l.k0);
        int p = 0;
#pragma unroll
        for (int i = 0; i < M; ++i) {
#pragma unroll
            for (int j = i + 1; j < M; ++j, ++p) {
                const float4 w = diced ? f4_mul(gh, dice4(a, key, b, C, p, l.k0)) : gh;
                const float4 rw = f4_scale(w, a.r_mf[p]);
                tm[i] = f4_fma4(rw, e[j], tm[i]);
                tm[j] = f4_fma4(rw, e[i], tm[j]);
                acc[p] += f4_dot(w, f4_mul(e[i], e[j]));
            }
        }
        float* dxb = dx + (size_t)b * a.F * a.K + l.k0;
        const float* xb = a.x + (size_t)b * a.F * a.K + l.k0;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const float4 w = diced ? f4_mul(gh, dice4(a, key, b, C, P + m, l.k0)) : gh;
            acc[P + m] += f4_dot(w, sq_minus(e[m], q[m]));
            const float4 s = f4_scale(w, 2.f * a.r_fm[m]);
            for (int i = a.plan.start[m]; i < a.plan.start[m + 1]; ++i) {
                const size_t o = (size_t)a.plan.order[i] * a.K;
                const float4 v = *reinterpret_cast<const float4*>(xb + o);
                *reinterpret_cast<float4*>(dxb + o) = f4_fma4(s, f4_sub(e[m], v), tm[m]);
            }
        }
    }

    // the workgroup's partial row: lane by lane, in lane order (an idle lane holds zeros)
    float* mine = sums + threadIdx.x * kLd;
#pragma unroll
    for (int c = 0; c < C; ++c) mine[c] = acc[c];
    mine[C] = db.x, mine[C + 1] = db.y, mine[C + 2] = db.z, mine[C + 3] = db.w;
    __syncthreads();
    float* row = rows + (size_t)blockIdx.x * (C + a.K);
    for (int c = threadIdx.x; c < C + a.K; c += kLanes) {
        float s = 0.f;
        if (c < C) {
            for (int ln = 0; ln < kLanes; ++ln) s += sums[ln * kLd + c];
        } else {
            const int k = c - C, chunk = k >> 2, comp = k & 3;
            for (int sl = 0; sl < T; ++sl) s += sums[(sl * kv + chunk) * kLd + C + comp];
        }
        row[c] = s;
    }
}

template <int M>
void launch_fwd(const FlArgs& a, const float* bias, float* e, float* h, hipStream_t st) {
    if (recalgo_drop::enabled(a.dice)) hipLaunchKernelGGL((flen_fwd_kernel<M, true>), dim3(workgroups(a.B, a.K)), dim3(kLanes), 0, st, a, bias, e, h);
    else hipLaunchKernelGGL((flen_fwd_kernel<M, false>), dim3(workgroups(a.B, a.K)), dim3(kLanes), 0, st, a, bias, e, h);
}
template <int M>
void launch_bwd(const FlArgs& a, const float* g_e, const float* g_h, float* dx, float* rows, hipStream_t st) {
    if (recalgo_drop::enabled(a.dice)) hipLaunchKernelGGL((flen_bwd_kernel<M, true>), dim3(workgroups(a.B, a.K)), dim3(kLanes), 0, st, a, g_e, g_h, dx, rows);
    else hipLaunchKernelGGL((flen_bwd_kernel<M, false>), dim3(workgroups(a.B, a.K)), dim3(kLanes), 0, st, a, g_e, g_h, dx, rows);
}

// what both entries check of the Dicefactor descriptor
bool dice_ok(const recalgo_dropout_t* d, int B, int M, int K) {
    if (d == nullptr) return true;
    const unsigned long long n = (unsigned long long)B * (M * (M - 1) / 2 + M) * K;
    return recalgo_drop::abi_ok(d) && n < (1ull << 32);
}

}  // namespace

RECALGO_EXPORT int recalgo_flen_abi_version(void) { return RECALGO_FLEN_ABI_VERSION; }

RECALGO_EXPORT int recalgo_flen_supported(int F, int M, int K) { return shape_ok(F, M, K) ? 1 : 0; }

RECALGO_EXPORT int recalgo_flen_bwd_partial_rows(int B, int F, int M, int K) {
    if (B < 1 || !shape_ok(F, M, K)) return 0;
    return workgroups(B, K);
}

RECALGO_EXPORT int64_t recalgo_flen_bwd_workspace_bytes(int B, int F, int M, int K) {
    if (B < 1 || !shape_ok(F, M, K)) return 0;
    return (int64_t)sizeof(float) * workgroups(B, K) * (M * (M - 1) / 2 + M + K);
}

RECALGO_EXPORT int recalgo_flen_fwd(const float* x, const int32_t* group_of, const float* r_mf, const float* r_fm, const float* bias,
                                    const void* dice, int B, int F, int M, int K, float* e, float* h, recalgo_stream_t stream) {
    const recalgo_dropout_t* d = static_cast<const recalgo_dropout_t*>(dice);
    RECALGO_REQUIRE(B >= 1 && shape_ok(F, M, K));
    RECALGO_REQUIRE(x && group_of && r_mf && r_fm && bias && e && h);
    RECALGO_REQUIRE(aligned16(x, e, h) && aligned_to<4>(r_mf, r_fm, bias) && dice_ok(d, B, M, K));
    FlArgs a = {x, r_mf, r_fm, B, F, K, recalgo_drop::from_abi(d), {}};
    RECALGO_REQUIRE(make_plan(group_of, F, M, &a.plan));
    hipStream_t st = as_stream(stream);
    switch (M) {
        case 2: launch_fwd<2>(a, bias, e, h, st); break;
        case 3: launch_fwd<3>(a, bias, e, h, st); break;
        case 4: launch_fwd<4>(a, bias, e, h, st); break;
        case 5: launch_fwd<5>(a, bias, e, h, st); break;
        case 6: launch_fwd<6>(a, bias, e, h, st); break;
        case 7: launch_fwd<7>(a, bias, e, h, st); break;
        default: launch_fwd<8>(a, bias, e, h, st); break;
    }
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_flen_bwd(const float* g_e, const float* g_h, const float* x, const int32_t* group_of, const float* r_mf,
                                    const float* r_fm, const void* dice, int B, int F, int M, int K, float* dx, float* dr_mf,
                                    float* dr_fm, float* dbias, void* workspace, recalgo_stream_t stream) {
    const recalgo_dropout_t* d = static_cast<const recalgo_dropout_t*>(dice);
    RECALGO_REQUIRE(B >= 1 && shape_ok(F, M, K));
    RECALGO_REQUIRE(g_e && g_h && x && group_of && r_mf && r_fm && dx && dr_mf && dr_fm && dbias && workspace);
    RECALGO_REQUIRE(aligned16(g_e, g_h, x, dx) && aligned_to<4>(r_mf, r_fm, dr_mf, dr_fm, dbias) && aligned_to<4>(workspace) &&
                    dice_ok(d, B, M, K));
    FlArgs a = {x, r_mf, r_fm, B, F, K, recalgo_drop::from_abi(d), {}};
    RECALGO_REQUIRE(make_plan(group_of, F, M, &a.plan));
    hipStream_t st = as_stream(stream);
    float* rows = static_cast<float*>(workspace);
    switch (M) {
        case 2: launch_bwd<2>(a, g_e, g_h, dx, rows, st); break;
        case 3: launch_bwd<3>(a, g_e, g_h, dx, rows, st); break;
        case 4: launch_bwd<4>(a, g_e, g_h, dx, rows, st); break;
        case 5: launch_bwd<5>(a, g_e, g_h, dx, rows, st); break;
        case 6: launch_bwd<6>(a, g_e, g_h, dx, rows, st); break;
        case 7: launch_bwd<7>(a, g_e, g_h, dx, rows, st); break;
        default: launch_bwd<8>(a, g_e, g_h, dx, rows, st); break;
    }
    const int P = M * (M - 1) / 2;
    float* const outs[3] = {dr_mf, dr_fm, dbias};
    const int starts[4] = {0, P, P + M, P + M + K};
    return recalgo_slabs::launch_colsums(rows, workgroups(B, K), 3, outs, starts, st);
}
