// DIEN's interest module (algorithm/DIEN/dien.py:196-229, custom_grucell.py): the GRU recurrence, and attention + the AGRU /
// AUGRU recurrence, two launches each way; include/recalgo_dien.h states the contract, DESIGN.md §5 "DIEN interest
// evolution" the layout and its t_min.
//
// Shape of all four kernels: a GROUP of G = 8 (nh <= 8) or 16 lanes works on one example, lane j of the group owns unit j
// of the state; a 256-thread workgroup holds 256 / G groups, all inside one wave each, so the chain of T dependent steps
// never meets a workgroup barrier: what a step exchanges between the units of an example (the state, r * h, the gate
// gradients) goes through a few doubles of LDS per group, fenced by wave_sync().  The weights (at most 1584 floats) are
// staged in LDS once per workgroup and read as broadcasts (every group reads the same address, the lanes of a group
// consecutive columns).  The input half of both products does not depend on the state: the row of step t + 1 is loaded
// while step t computes.  A wave runs the steps up to the longest history of its groups; a shorter one is predicated.
//
// Arithmetic: every product, sigmoid, tanh and exp is evaluated in double and the state is rounded to fp32 once per step,
// when it is stored — the value the next step and the backward's recomputation both read.  A chain of 64 steps in fp32
// would add its roundings up; the library's parity policy (tests/util.py) counts elements against the fp32 reference.
// The backward kernels recompute the gates of step t from the stored state of step t - 1 and keep every parameter gradient in
// registers (doubles, added over the steps and the examples in a fixed order): a backward group is twice as wide, the second
// half being helper lanes that own a third of the columns (see Acc).  The groups' registers are added in group order through
// LDS into one partial row per workgroup; recalgo_slabs::launch_colsums adds the rows in the fixed order of slab_sum.h.
// No float atomics.  The kernels are instantiated per nh (4, 8, 12, 16): every loop over the units unrolls.
#include "common.h"
#include "slab_sum.h"

#include "../../include/recalgo_dien.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxT = RECALGO_DIEN_MAX_T, kMaxNA = RECALGO_DIEN_MAX_NA, kMaxNH = RECALGO_DIEN_MAX_NH;
constexpr int kBwdRows = 256;                        // cap of the backward grids: one workgroup per CU
constexpr float kMaskValue = -4294967296.0f;         // float32(-2^32 + 1)
constexpr int kMaxWeights = (kMaxNA + kMaxNH) * 3 * kMaxNH + 3 * kMaxNH;      // Wg | bg | Wc | bc of the widest cell
constexpr int kMaxAcc = kMaxWeights + kMaxNH * kMaxNA;                         // + dw_att: the widest partial row

template <int NH>
struct Geo {
    static constexpr int G = NH <= 8 ? 8 : 16;       // lanes of a group
    static constexpr int SLOTS = kThreads / G;       // groups of a workgroup
};

// what the units of one example exchange during a step
template <int NH>
struct Slot {
    double H[NH], RH[NH], DC[NH], DG[2 * NH], DE[NH];
};

struct Cell {
    const float *Wg, *bg, *Wc, *bc;
};

template <int W>
__device__ __forceinline__ double group_sum_d(double v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ double sigmoid_d(double v) { return 1.0 / (1.0 + exp(-v)); }

__device__ __forceinline__ int clamped(const int32_t* lengths, int e, int T) {
    if (lengths == nullptr) return T;
    const int l = lengths[e];
    return l < 0 ? 0 : (l > T ? T : l);
}

// sW <- Wg | bg | Wc | bc of a cell whose input is nx wide
template <int NH>
__device__ __forceinline__ void stage_cell(float* sW, const Cell& w, int nx) {
    const int ng = (nx + NH) * 2 * NH, nc = (nx + NH) * NH;
    for (int i = threadIdx.x; i < ng; i += kThreads) sW[i] = w.Wg[i];
    for (int i = threadIdx.x; i < 2 * NH; i += kThreads) sW[ng + i] = w.bg[i];
    for (int i = threadIdx.x; i < nc; i += kThreads) sW[ng + 2 * NH + i] = w.Wc[i];
    for (int i = threadIdx.x; i < NH; i += kThreads) sW[ng + 2 * NH + nc + i] = w.bc[i];
}

// the nx <= NX floats of a row, the same for every lane of the group
template <int NX>
__device__ __forceinline__ void load_row(float (&r)[NX], const float* __restrict__ p, int nx) {
#pragma unroll
    for (int k = 0; k < NX; ++k) r[k] = k < nx ? p[k] : 0.f;
}

// r, u, c of one step for unit j (jj = j for a unit lane, 0 for an idle one: its results are not used).  Leaves H = the
// state and RH = r * h of the whole example in the slot.  Two wave_sync()s.
template <int NH, int NX>
__device__ __forceinline__ void cell_gates(const float* sW, int nx, const float (&x)[NX], Slot<NH>& S, int j, bool unit, double hj,
                                           double& r, double& u, double& c) {
    const float* Wg = sW;
    const float* bg = Wg + (nx + NH) * 2 * NH;
    const float* Wc = bg + 2 * NH;
    const float* bc = Wc + (nx + NH) * NH;
    const int jj = unit ? j : 0;
    double pr = (double)bg[jj], pu = (double)bg[NH + jj], pc = (double)bc[jj];
#pragma unroll
    for (int k = 0; k < NX; ++k) {
        if (k < nx) {
            const double xv = (double)x[k];
            pr = fma(xv, (double)Wg[k * 2 * NH + jj], pr);
            pu = fma(xv, (double)Wg[k * 2 * NH + NH + jj], pu);
            pc = fma(xv, (double)Wc[k * NH + jj], pc);
        }
    }
    if (unit) S.H[j] = hj;
    wave_sync();
#pragma unroll
    for (int k = 0; k < NH; ++k) {
        const double hv = S.H[k];
        pr = fma(hv, (double)Wg[(nx + k) * 2 * NH + jj], pr);
        pu = fma(hv, (double)Wg[(nx + k) * 2 * NH + NH + jj], pu);
    }
    r = sigmoid_d(pr), u = sigmoid_d(pu);
    if (unit) S.RH[j] = r * hj;
    wave_sync();
#pragma unroll
    for (int k = 0; k < NH; ++k) pc = fma(S.RH[k], (double)Wc[(nx + k) * NH + jj], pc);
    c = tanh(pc);
}

__device__ __forceinline__ double next_state(int mode, double a, double h, double u, double c) {
    if (mode == RECALGO_DIEN_MODE_GRU) return u * h + (1.0 - u) * c;
    if (mode == RECALGO_DIEN_MODE_AGRU) return (1.0 - a) * h + a * c;
    const double up = (1.0 - a) * u;
    return up * h + (1.0 - up) * c;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
template <int NH>
__global__ __launch_bounds__(kThreads) void dien_gru_fwd_kernel(const float* __restrict__ x, const int32_t* __restrict__ lengths, Cell w,
                                                                int B, int T, int na, float* __restrict__ h) {
    constexpr int G = Geo<NH>::G, SLOTS = Geo<NH>::SLOTS;
    __shared__ float sW[kMaxWeights];
    __shared__ Slot<NH> sS[SLOTS];
    stage_cell<NH>(sW, w, na);
    __syncthreads();
    const int slot = threadIdx.x / G, j = threadIdx.x % G;
    const bool unit = j < NH;
    const int e = blockIdx.x * SLOTS + slot;
    const bool valid = e < B;
    const int L = valid ? clamped(lengths, e, T) : 0;
    const int tmax = wave_max_i(L);
    const float* xe = x + (size_t)(valid ? e : 0) * T * na;
    float* he = h + (size_t)(valid ? e : 0) * T * NH;
    Slot<NH>& S = sS[slot];
    double hj = 0.0;
    float xn[kMaxNA];
    load_row(xn, xe, tmax > 0 ? na : 0);
    for (int t = 0; t < tmax; ++t) {
        float xc[kMaxNA];
#pragma unroll
        for (int k = 0; k < kMaxNA; ++k) xc[k] = xn[k];
        if (t + 1 < tmax) load_row(xn, xe + (size_t)(t + 1) * na, na);
        double r, u, c;
        cell_gates<NH, kMaxNA>(sW, na, xc, S, j, unit, hj, r, u, c);
        const float hf = (float)next_state(RECALGO_DIEN_MODE_GRU, 0.0, hj, u, c);
        const bool act = t < L;
        if (valid && unit) he[t * NH + j] = act ? hf : 0.f;
        if (act) hj = (double)hf;
    }
    if (valid && unit)
        for (int t = tmax; t < T; ++t) he[t * NH + j] = 0.f;
}

// e_j = sum_k w_att[j, k] target[k]
__device__ __forceinline__ double projected_target(const float* __restrict__ w_att, const float* __restrict__ tg, int na, int j) {
    double s = 0.0;
    for (int k = 0; k < na; ++k) s = fma((double)w_att[j * na + k], (double)tg[k], s);
    return s;
}

template <int NH>
__global__ __launch_bounds__(kThreads) void dien_evolve_fwd_kernel(const float* __restrict__ h, const float* __restrict__ target,
                                                                   const int32_t* __restrict__ lengths,
                                                                   const float* __restrict__ w_att, Cell w, int B, int T, int na,
                                                                   int mode, float* __restrict__ att, float* __restrict__ states,
                                                                   float* __restrict__ final_state) {
    constexpr int G = Geo<NH>::G, SLOTS = Geo<NH>::SLOTS;
    __shared__ float sW[kMaxWeights];
    __shared__ Slot<NH> sS[SLOTS];
    __shared__ float sA[SLOTS][kMaxT];               // the scores, then the attention weights
    __shared__ double sE[SLOTS][kMaxT];              // exp(score - max)
    stage_cell<NH>(sW, w, NH);
    __syncthreads();
    const int slot = threadIdx.x / G, j = threadIdx.x % G;
    const bool unit = j < NH;
    const int e = blockIdx.x * SLOTS + slot;
    const bool valid = e < B;
    const int ee = valid ? e : 0;
    const int L = valid ? clamped(lengths, e, T) : 0;
    const int tmax = wave_max_i(L);
    const float* he = h + (size_t)ee * T * NH;
    Slot<NH>& S = sS[slot];
    float* A = sA[slot];
    // scores: s[t] = h[t] . (w_att target), replaced past L
    const double ej = unit ? projected_target(w_att, target + (size_t)ee * na, na, j) : 0.0;
    for (int t = 0; t < T; ++t) {
        const double p = group_sum_d<G>(unit ? (double)he[t * NH + j] * ej : 0.0);
        if (j == 0) A[t] = t < L ? (float)p : kMaskValue;
    }
    wave_sync();
    // softmax: lane j takes the entries j, j + G, ..; the sum is taken entry by entry in t order (a replaced entry adds an
    // exact 0, so a padded T changes no bit)
    float m = -INFINITY;
    for (int t = j; t < T; t += G) m = fmaxf(m, A[t]);
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    double* E = sE[slot];
    for (int t = j; t < T; t += G) E[t] = exp((double)(A[t] - m));
    wave_sync();
    double sum = 0.0;
    for (int t = 0; t < T; ++t) sum += E[t];
    for (int t = j; t < T; t += G) {
        const float a = (float)(E[t] / sum);
        A[t] = a;
        if (valid) att[(size_t)e * T + t] = a;
    }
    wave_sync();
    // the recurrence over the rows of h
    float* se = states + (size_t)ee * T * NH;
    double hj = 0.0;
    float xn[NH];
    load_row(xn, he, tmax > 0 ? NH : 0);
    for (int t = 0; t < tmax; ++t) {
        float xc[NH];
#pragma unroll
        for (int k = 0; k < NH; ++k) xc[k] = xn[k];
        if (t + 1 < tmax) load_row(xn, he + (size_t)(t + 1) * NH, NH);
        double r, u, c;
        cell_gates<NH, NH>(sW, NH, xc, S, j, unit, hj, r, u, c);
        const float hf = (float)next_state(mode, (double)A[t], hj, u, c);
        const bool act = t < L;
        if (valid && unit) se[t * NH + j] = act ? hf : 0.f;
        if (act) hj = (double)hf;
    }
    if (valid && unit) {
        for (int t = tmax; t < T; ++t) se[t * NH + j] = 0.f;
        final_state[(size_t)e * NH + j] = (float)hj;
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// A backward group is twice as wide as a forward one: lanes [0, GU) are the units, as in the forward; lane GU + j is the
// HELPER of unit j.  Both run the chain; they share the parameter gradients of column j: the unit keeps Wg's r half and Wc
// (a1, a2; rows: NX of the input, NH of the state) with their bias elements, the helper Wg's u half (a1) and its bias element.
// (One lane holding all three columns of the widest cell needs more registers than a lane has.)
template <int NH, int NX>
struct Acc {
    double a1[NX + NH], a2[NX + NH], b1, b2;
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int k = 0; k < NX + NH; ++k) a1[k] = a2[k] = 0.0;
        b1 = b2 = 0.0;
    }
};

// One step of the chain backwards.  dh: the gradient of the step's new state (0 on a predicated step: every result is then
// an exact zero); hj: unit j of the state the step started from; returns in `carry` the gradient of that state, in dxk the
// lane's element j of the input row's gradient (G >= NX), in da the lane's share of the attention weight's gradient.
// Five wave_sync()s.
template <int NH, int NX, int G>
__device__ __forceinline__ void cell_bwd_step(const float* sW, int nx, const float (&x)[NX], Slot<NH>& S, int j, bool unit, int mode,
                                              double a, double hj, double dh, Acc<NH, NX>& acc, double& carry, double& da,
                                              double& dxk) {
    static_assert(G >= NX && G >= 2 * NH, "a backward group covers the input row and holds a helper per unit");
    constexpr int GU = G / 2;
    const float* Wg = sW;
    const float* Wc = Wg + (nx + NH) * 2 * NH + 2 * NH;
    const int jj = unit ? j : 0;
    double r, u, c;
    cell_gates<NH, NX>(sW, nx, x, S, j, unit, hj, r, u, c);
    double du = 0.0, dc, cn;
    da = 0.0;
    if (mode == RECALGO_DIEN_MODE_GRU) {
        du = dh * (hj - c), dc = dh * (1.0 - u), cn = dh * u;
    } else if (mode == RECALGO_DIEN_MODE_AGRU) {
        dc = dh * a, cn = dh * (1.0 - a), da = dh * (c - hj);
    } else {
        const double up = (1.0 - a) * u, dup = dh * (hj - c);
        dc = dh * (1.0 - up), cn = dh * up, da = -dup * u, du = dup * (1.0 - a);
    }
    const double dcp = dc * (1.0 - c * c), dgu = du * u * (1.0 - u);
    if (unit) S.DC[j] = dcp, S.DG[NH + j] = dgu;
    wave_sync();
    double drh = 0.0;
#pragma unroll
    for (int m = 0; m < NH; ++m) drh = fma(S.DC[m], (double)Wc[(nx + jj) * NH + m], drh);
    const double dgr = drh * hj * r * (1.0 - r);
    cn = fma(drh, r, cn);
    if (unit) S.DG[j] = dgr;
    wave_sync();
#pragma unroll
    for (int m = 0; m < 2 * NH; ++m) cn = fma(S.DG[m], (double)Wg[(nx + jj) * 2 * NH + m], cn);
    carry = cn;
    dxk = 0.0;
    if (j < nx) {
#pragma unroll
        for (int m = 0; m < NH; ++m) dxk = fma(S.DC[m], (double)Wc[j * NH + m], dxk);
#pragma unroll
        for (int m = 0; m < 2 * NH; ++m) dxk = fma(S.DG[m], (double)Wg[j * 2 * NH + m], dxk);
    }
    const bool helper = j >= GU && j - GU < NH;
    if (unit || helper) {
        const double v1 = helper ? S.DG[NH + (helper ? j - GU : 0)] : dgr, v2 = helper ? 0.0 : dcp;       // (a helper's a2 stays 0)
#pragma unroll
        for (int k = 0; k < NX; ++k) {
            if (k < nx) {
                const double xv = (double)x[k];
                acc.a1[k] = fma(xv, v1, acc.a1[k]), acc.a2[k] = fma(xv, v2, acc.a2[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < NH; ++k) {
            acc.a1[NX + k] = fma(S.H[k], v1, acc.a1[NX + k]), acc.a2[NX + k] = fma(S.RH[k], v2, acc.a2[NX + k]);
        }
        acc.b1 += v1, acc.b2 += v2;
    }
    wave_sync();            // (the next step overwrites H and RH)
}

// red[..] += the lane's accumulators, laid out as the header's Wg | bg | Wc | bc of a cell with an nx-wide input; `col` is
// the lane's column, `helper` says which of the two roles it has
template <int NH, int NX>
__device__ __forceinline__ void add_cell_acc(double* red, const Acc<NH, NX>& acc, int nx, int col, bool helper) {
    double* g = red + (helper ? NH : 0);
    double* bg = red + (nx + NH) * 2 * NH + (helper ? NH : 0);
    double* cc = red + (nx + NH) * 2 * NH + 2 * NH;
    double* bc = cc + (nx + NH) * NH;
#pragma unroll
    for (int k = 0; k < NX; ++k) {
        if (k < nx) {
            g[k * 2 * NH + col] += acc.a1[k];
            if (!helper) cc[k * NH + col] += acc.a2[k];
        }
    }
#pragma unroll
    for (int k = 0; k < NH; ++k) {
        g[(nx + k) * 2 * NH + col] += acc.a1[NX + k];
        if (!helper) cc[(nx + k) * NH + col] += acc.a2[NX + k];
    }
    bg[col] += acc.b1;
    if (!helper) bc[col] += acc.b2;
}

template <int NH>
__global__ __launch_bounds__(kThreads) void dien_gru_bwd_kernel(const float* __restrict__ x, const int32_t* __restrict__ lengths,
                                                                const float* __restrict__ h, Cell w, const float* __restrict__ g_h,
                                                                int B, int T, int na, float* __restrict__ dx,
                                                                float* __restrict__ partials) {
    constexpr int G = 2 * Geo<NH>::G, SLOTS = kThreads / G, NX = kMaxNA;
    __shared__ float sW[kMaxWeights];
    __shared__ Slot<NH> sS[SLOTS];
    __shared__ double sRed[kMaxAcc];
    const int n_acc = (na + NH) * 3 * NH + 3 * NH;
    stage_cell<NH>(sW, w, na);
    for (int i = threadIdx.x; i < n_acc; i += kThreads) sRed[i] = 0.0;
    __syncthreads();
    const int slot = threadIdx.x / G, j = threadIdx.x % G, rows = gridDim.x;
    const bool unit = j < NH;
    Slot<NH>& S = sS[slot];
    Acc<NH, NX> acc;
    acc.clear();
    for (int first = blockIdx.x; first < B; first += rows * SLOTS) {          // (the same for the whole workgroup)
        const int e = first + rows * slot;
        const bool valid = e < B;
        const int ee = valid ? e : 0;
        const int L = valid ? clamped(lengths, e, T) : 0;
        const int tmax = wave_max_i(L);
        const float* xe = x + (size_t)ee * T * na;
        const float* he = h + (size_t)ee * T * NH;
        const float* ge = g_h + (size_t)ee * T * NH;
        float* dxe = dx + (size_t)ee * T * na;
        if (valid)
            for (int t = tmax; t < T; ++t)
                for (int k = j; k < na; k += G) dxe[t * na + k] = 0.f;
        double carry = 0.0;
        for (int t = tmax - 1; t >= 0; --t) {
            const bool act = t < L;
            float xc[NX];
            load_row(xc, xe + (size_t)t * na, act ? na : 0);          // (a predicated step reads no row: see the header)
            const double hj = (unit && t > 0) ? (double)he[(t - 1) * NH + j] : 0.0;
            const double dh = (act && unit) ? (double)ge[t * NH + j] + carry : 0.0;
            double cn, da, dxk;
            cell_bwd_step<NH, NX, G>(sW, na, xc, S, j, unit, RECALGO_DIEN_MODE_GRU, 0.0, hj, dh, acc, cn, da, dxk);
            if (act) carry = cn;
            if (valid && j < na) dxe[t * na + j] = act ? (float)dxk : 0.f;
        }
    }
    // the groups' registers, added in group order (a unit and its helper own different columns)
    const bool helper = j >= G / 2 && j - G / 2 < NH;
    for (int s = 0; s < SLOTS; ++s) {
        if (slot == s && (unit || helper)) add_cell_acc<NH, NX>(sRed, acc, na, helper ? j - G / 2 : j, helper);
        __syncthreads();
    }
    float* prow = partials + (size_t)blockIdx.x * n_acc;
    for (int i = threadIdx.x; i < n_acc; i += kThreads) prow[i] = (float)sRed[i];
}

template <int NH>
__global__ __launch_bounds__(kThreads) void dien_evolve_bwd_kernel(const float* __restrict__ h, const float* __restrict__ target,
                                                                   const int32_t* __restrict__ lengths,
                                                                   const float* __restrict__ w_att, Cell w,
                                                                   const float* __restrict__ att, const float* __restrict__ states,
                                                                   const float* __restrict__ g_final, int B, int T, int na, int mode,
                                                                   float* __restrict__ dh_out, float* __restrict__ dtarget,
                                                                   float* __restrict__ partials) {
    constexpr int G = 2 * Geo<NH>::G, SLOTS = kThreads / G, NX = NH;
    __shared__ float sW[kMaxWeights];
    __shared__ Slot<NH> sS[SLOTS];
    __shared__ double sDA[SLOTS][kMaxT];             // d loss / d att[t] of the slot's example
    __shared__ double sRed[kMaxAcc];
    const int n_att = NH * na, n_acc = n_att + 2 * NH * 3 * NH + 3 * NH;
    stage_cell<NH>(sW, w, NH);
    for (int i = threadIdx.x; i < n_acc; i += kThreads) sRed[i] = 0.0;
    __syncthreads();
    const int slot = threadIdx.x / G, j = threadIdx.x % G, rows = gridDim.x;
    const bool unit = j < NH;
    Slot<NH>& S = sS[slot];
    double* DA = sDA[slot];
    Acc<NH, NX> acc;
    acc.clear();
    double aw[kMaxNA];                               // row j of dw_att
#pragma unroll
    for (int k = 0; k < kMaxNA; ++k) aw[k] = 0.0;
    for (int first = blockIdx.x; first < B; first += rows * SLOTS) {
        const int e = first + rows * slot;
        const bool valid = e < B;
        const int ee = valid ? e : 0;
        const int L = valid ? clamped(lengths, e, T) : 0;
        const int tmax = wave_max_i(L);
        const float* he = h + (size_t)ee * T * NH;
        const float* se = states + (size_t)ee * T * NH;
        const float* ae = att + (size_t)ee * T;
        const float* tg = target + (size_t)ee * na;
        float* dhe = dh_out + (size_t)ee * T * NH;
        if (valid && unit)
            for (int t = L; t < T; ++t) dhe[t * NH + j] = 0.f;
        double carry = (valid && unit) ? (double)g_final[(size_t)e * NH + j] : 0.0;
        for (int t = tmax - 1; t >= 0; --t) {
            const bool act = t < L;
            float xc[NX];
            load_row(xc, he + (size_t)t * NH, act ? NH : 0);
            const double a = (double)ae[t];
            const double hj = (unit && t > 0) ? (double)se[(t - 1) * NH + j] : 0.0;
            const double dh = (act && unit) ? carry : 0.0;
            double cn, da, dxk;
            cell_bwd_step<NH, NX, G>(sW, NH, xc, S, j, unit, mode, a, hj, dh, acc, cn, da, dxk);
            if (act) carry = cn;
            da = group_sum_d<G>(da);
            if (j == 0) DA[t] = da;
            if (act && unit) dhe[t * NH + j] = (float)dxk;          // the cell-input path; the score path is added below
        }
        wave_sync();
        // the softmax backwards over the L entries that are not replaced, then s[t] = h[t] . e
        double dot = 0.0;
        for (int t = 0; t < L; ++t) dot = fma((double)ae[t], DA[t], dot);
        const double ej = unit ? projected_target(w_att, tg, na, j) : 0.0;
        double de = 0.0;
        if (unit) {
            for (int t = 0; t < L; ++t) {
                const double ds = (double)ae[t] * (DA[t] - dot);
                de = fma(ds, (double)he[t * NH + j], de);
                dhe[t * NH + j] = (float)((double)dhe[t * NH + j] + ds * ej);
            }
#pragma unroll
            for (int k = 0; k < kMaxNA; ++k)
                if (k < na) aw[k] = fma(de, (double)tg[k], aw[k]);
            S.DE[j] = de;
        }
        wave_sync();
        if (valid) {
            for (int k = j; k < na; k += G) {
                double s = 0.0;
#pragma unroll
                for (int m = 0; m < NH; ++m) s = fma(S.DE[m], (double)w_att[m * na + k], s);
                dtarget[(size_t)e * na + k] = (float)s;
            }
        }
        wave_sync();        // (the next example overwrites DE and DA)
    }
    const bool helper = j >= G / 2 && j - G / 2 < NH;
    for (int s = 0; s < SLOTS; ++s) {
        if (slot == s && unit) {
#pragma unroll
            for (int k = 0; k < kMaxNA; ++k)
                if (k < na) sRed[j * na + k] += aw[k];
        }
        if (slot == s && (unit || helper)) add_cell_acc<NH, NX>(sRed + n_att, acc, NH, helper ? j - G / 2 : j, helper);
        __syncthreads();
    }
    float* prow = partials + (size_t)blockIdx.x * n_acc;
    for (int i = threadIdx.x; i < n_acc; i += kThreads) prow[i] = (float)sRed[i];
}

bool width_ok(int n, int cap) { return n >= 4 && n <= cap && (n & 3) == 0; }

bool shape_ok(int T, int na, int nh) { return T >= 1 && T <= kMaxT && width_ok(na, kMaxNA) && width_ok(nh, kMaxNH); }

int rows_for(int B) { return B < 1 ? 1 : (B > kBwdRows ? kBwdRows : B); }

int slots_of(int nh) { return kThreads / (nh <= 8 ? 8 : 16); }

int gru_row(int na, int nh) { return (na + nh) * 3 * nh + 3 * nh; }

int evolve_row(int na, int nh) { return nh * na + 2 * nh * 3 * nh + 3 * nh; }

// nh is one of 4, 8, 12, 16 (shape_ok)
#define DIEN_LAUNCH(KERNEL, nh, grid, st, ...)                                                             \
    do {                                                                                                   \
        if ((nh) == 4) hipLaunchKernelGGL(KERNEL<4>, grid, dim3(kThreads), 0, st, __VA_ARGS__);            \
        else if ((nh) == 8) hipLaunchKernelGGL(KERNEL<8>, grid, dim3(kThreads), 0, st, __VA_ARGS__);       \
        else if ((nh) == 12) hipLaunchKernelGGL(KERNEL<12>, grid, dim3(kThreads), 0, st, __VA_ARGS__);     \
        else hipLaunchKernelGGL(KERNEL<16>, grid, dim3(kThreads), 0, st, __VA_ARGS__);                     \
    } while (0)

}  // namespace

RECALGO_EXPORT int recalgo_dien_abi_version(void) { return RECALGO_DIEN_ABI_VERSION; }

RECALGO_EXPORT int recalgo_dien_supported(int T, int na, int nh) { return shape_ok(T, na, nh) ? 1 : 0; }

RECALGO_EXPORT int recalgo_dien_gru_bwd_partial_rows(int B) { return rows_for(B); }

RECALGO_EXPORT int64_t recalgo_dien_gru_bwd_workspace_bytes(int B, int na, int nh) {
    if (!shape_ok(1, na, nh)) return 0;
    return (int64_t)sizeof(float) * rows_for(B) * gru_row(na, nh);
}

RECALGO_EXPORT int recalgo_dien_evolve_bwd_partial_rows(int B) { return rows_for(B); }

RECALGO_EXPORT int64_t recalgo_dien_evolve_bwd_workspace_bytes(int B, int na, int nh) {
    if (!shape_ok(1, na, nh)) return 0;
    return (int64_t)sizeof(float) * rows_for(B) * evolve_row(na, nh);
}

RECALGO_EXPORT int recalgo_dien_gru_fwd(const float* x, const int32_t* lengths, const float* Wg, const float* bg, const float* Wc,
                                        const float* bc, int B, int T, int na, int nh, float* h, recalgo_stream_t stream) {
    RECALGO_REQUIRE(B >= 1 && shape_ok(T, na, nh));
    RECALGO_REQUIRE(x && Wg && bg && Wc && bc && h);
    RECALGO_REQUIRE(aligned_to<4>(x, Wg, bg, Wc, bc, h) && aligned_to<4>(lengths));
    const Cell w = {Wg, bg, Wc, bc};
    DIEN_LAUNCH(dien_gru_fwd_kernel, nh, dim3(cdiv(B, slots_of(nh))), as_stream(stream), x, lengths, w, B, T, na, h);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_dien_gru_bwd(const float* x, const int32_t* lengths, const float* h, const float* Wg, const float* bg,
                                        const float* Wc, const float* bc, const float* g_h, int B, int T, int na, int nh,
                                        float* dx, float* dWg, float* dbg, float* dWc, float* dbc, float* workspace,
                                        recalgo_stream_t stream) {
    RECALGO_REQUIRE(B >= 1 && shape_ok(T, na, nh));
    RECALGO_REQUIRE(x && h && Wg && bg && Wc && bc && g_h && dx && dWg && dbg && dWc && dbc && workspace);
    RECALGO_REQUIRE(aligned_to<4>(x, h, Wg, bg, Wc, bc, g_h, dx, dWg, dbg, dWc, dbc, workspace) && aligned_to<4>(lengths));
    const Cell w = {Wg, bg, Wc, bc};
    const int rows = rows_for(B), n = gru_row(na, nh);
    hipStream_t st = as_stream(stream);
    DIEN_LAUNCH(dien_gru_bwd_kernel, nh, dim3(rows), st, x, lengths, h, w, g_h, B, T, na, dx, workspace);
    float* const outs[4] = {dWg, dbg, dWc, dbc};
    const int ng = (na + nh) * 2 * nh, nc = (na + nh) * nh;
    const int starts[5] = {0, ng, ng + 2 * nh, ng + 2 * nh + nc, n};
    return recalgo_slabs::launch_colsums(workspace, rows, 4, outs, starts, st);
}

RECALGO_EXPORT int recalgo_dien_evolve_fwd(const float* h, const float* target, const int32_t* lengths, const float* w_att,
                                           const float* Wg, const float* bg, const float* Wc, const float* bc, int B, int T, int na,
                                           int nh, int mode, float* att, float* states, float* final_state,
                                           recalgo_stream_t stream) {
    RECALGO_REQUIRE(B >= 1 && shape_ok(T, na, nh) && (mode == RECALGO_DIEN_MODE_AGRU || mode == RECALGO_DIEN_MODE_AUGRU));
    RECALGO_REQUIRE(h && target && lengths && w_att && Wg && bg && Wc && bc && att && states && final_state);
    RECALGO_REQUIRE(aligned_to<4>(h, target, w_att, Wg, bg, Wc, bc, att, states, final_state) && aligned_to<4>(lengths));
    const Cell w = {Wg, bg, Wc, bc};
    DIEN_LAUNCH(dien_evolve_fwd_kernel, nh, dim3(cdiv(B, slots_of(nh))), as_stream(stream), h, target, lengths, w_att, w, B, T, na,
                mode, att, states, final_state);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_dien_evolve_bwd(const float* h, const float* target, const int32_t* lengths, const float* w_att,
                                           const float* Wg, const float* bg, const float* Wc, const float* bc, const float* att,
                                           const float* states, const float* g_final, int B, int T, int na, int nh, int mode,
                                           float* dh, float* dtarget, float* dw_att, float* dWg, float* dbg, float* dWc, float* dbc,
                                           float* workspace, recalgo_stream_t stream) {
    RECALGO_REQUIRE(B >= 1 && shape_ok(T, na, nh) && (mode == RECALGO_DIEN_MODE_AGRU || mode == RECALGO_DIEN_MODE_AUGRU));
    RECALGO_REQUIRE(h && target && lengths && w_att && Wg && bg && Wc && bc && att && states && g_final);
    RECALGO_REQUIRE(dh && dtarget && dw_att && dWg && dbg && dWc && dbc && workspace);
    RECALGO_REQUIRE(aligned_to<4>(h, target, w_att, Wg, bg, Wc, bc, att, states, g_final) && aligned_to<4>(lengths));
    RECALGO_REQUIRE(aligned_to<4>(dh, dtarget, dw_att, dWg, dbg, dWc, dbc, workspace));
    const Cell w = {Wg, bg, Wc, bc};
    const int rows = rows_for(B), n = evolve_row(na, nh);
    hipStream_t st = as_stream(stream);
    DIEN_LAUNCH(dien_evolve_bwd_kernel, nh, dim3(rows), st, h, target, lengths, w_att, w, att, states, g_final, B, T, na, mode, dh,
                dtarget, workspace);
    float* const outs[5] = {dw_att, dWg, dbg, dWc, dbc};
    const int na_ = nh * na, ng = 2 * nh * 2 * nh, nc = 2 * nh * nh;
    const int starts[6] = {0, na_, na_ + ng, na_ + ng + 2 * nh, na_ + ng + 2 * nh + nc, n};
    return recalgo_slabs::launch_colsums(workspace, rows, 5, outs, starts, st);
}
