// Held-out rows against M engines at once: the predictive averaged over the
// members of an ensemble.  Part of kernels.h.
//
// Per query row q and member e (an engine: one posterior sample of the
// partition and the hyper-parameters):
//   w[e][q]   = k_predict's logp of row q on member e, bit for bit; under
//               LowEntropy minus the member's prior total (log_sum_exp of its
//               driver scores alone), one float subtraction;
//   logp[q]   = log_sum_exp(w[0..M)[q]) - fast_log((float)M), log_sum_exp as
//               random.cc:78-92 has it: the maximum, the in-order float sum
//               of fast_exp(w - max), fast_log(total) + max;
//   member[q] = sample_from_scores_overwrite (random.hpp:361-366) over
//               w[.][q] with engine step draw_base + q + 1 of the member
//               stream, or the first maximum;
//   group[q]  = k_predict's group of row q on member member[q].
// Phase A (k_predict_many) writes the planes w, k_ensemble_fold folds them,
// phase B (k_predict_many_pick) draws the group in the chosen member only.
#pragma once

namespace dist {

// One member of the call, read from a device array by blockIdx.y (as
// ChainArgs by k_chains): everything k_predict takes as kernel arguments.
struct PredictMember {
    SweepParams P;
    PredictArgs A;       // phase A: logp = the member's plane, group = its
                         // plane of groups (draw-all form) or null
    PredictArgs B;       // phase B: logp = null, group = the call's output
    float * prior;       // [K] = A.prior, as k_predict_prior_many writes it
    float * total;       // the member's prior total, or null (not wanted)
    const float * sub;   // = total under LowEntropy, else null
};

// k_predict_prior for every member: grid (K blocks, M)
__global__ void k_predict_prior_many(const PredictMember * __restrict__ all) {
    const PredictMember & M = all[blockIdx.y];
    const SweepParams & P = M.P;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P.K) return;
    M.prior[k] = P.cluster == 1
        ? le_score_add_value(P.dataset_size, P.counts[k], (int)P.sample_size,
                             P.n_empty)
        : P.shifted[k] + P.scalars->shift_full;
}

// log_sum_exp of each member's driver scores alone (random.cc:78-92), the
// members side by side: sample_scalar's arithmetic, one lane per member
__global__ void k_predict_prior_totals(const PredictMember * __restrict__ all,
                                       int m) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m) return;
    const PredictMember & M = all[e];
    if (M.total == nullptr) return;
    SampleOut out;
    sample_scalar(2, M.P.K, M.prior, 0.f, 0.f, &out);
    *M.total = out.log_sum_exp;
}

// the ensemble kernels' copy of the exponential's table, as k_predict's
__device__ __forceinline__ void predict_load_exp(uint32_t * s_exp) {
    for (int i = threadIdx.x; i < 1024; i += kBlock)
        s_exp[i] = g_tables_dev.exp_table[i];
    __syncthreads();
}
// a member's logp: under LowEntropy minus its prior total (sub), else as it is
__device__ __forceinline__ float predict_minus(float lp, const float * sub) {
    return sub != nullptr ? lp - *sub : lp;
}

// Phase A: k_predict's passes 1 and 2 for every (member, row); grid (row
// blocks, M).  The member is wave-uniform, so are its parameters.
template <int KIND0, int KIND1, int NF>
__global__ __launch_bounds__(kBlock) void k_predict_many(
        const PredictMember * __restrict__ all) {
    __shared__ uint32_t s_exp[1024];
    predict_load_exp(s_exp);
    const PredictMember & M = all[blockIdx.y];
    const SweepParams & P = M.P;
    const PredictArgs & A = M.A;
    const float * const sub = M.sub;
#define PREDICT_COUNT P.row_end
#define PREDICT_FIRST (size_t)blockIdx.x * kBlock + threadIdx.x
#define PREDICT_STRIDE (size_t)gridDim.x * kBlock
#define PREDICT_ROW(item) item
#define PREDICT_LOGP(x) predict_minus(x, sub)
#include "kernels_predict_body.h"
#undef PREDICT_COUNT
#undef PREDICT_FIRST
#undef PREDICT_STRIDE
#undef PREDICT_ROW
#undef PREDICT_LOGP
}

// The fold over the members of `items` columns of the planes w[e][item]
// (ld >= items): a lane per item, members in index order, reads coalesced
// over the items.  (items, not rows: a plane may hold rows x candidates.)
struct EnsembleFold {
    const float * w;
    size_t ld;
    int m;
    size_t items;
    float * logp;              // [items] or null
    uint32_t * member;         // [items] or null
    int mode;                  // 0: draw, 1: first maximum
    // the member stream: item i draws with seed_batch * 16807^i
    uint32_t seed_batch;
    const uint32_t * pow_lo;
    const uint32_t * pow_hi;
    // draw-all form: group[item] = groups[member][item] (both or neither)
    const uint32_t * groups;
    size_t groups_ld;
    uint32_t * group;
};
__global__ __launch_bounds__(kBlock) void k_ensemble_fold(EnsembleFold A) {
    const size_t item = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (item >= A.items) return;
    const float * col = A.w + item;
    // vector_max (vector_math.cc:74-83) and the first index that attains it
    float mx = col[0];
    int arg = 0;
    for (int e = 0; e < A.m; ++e) {
        const float x = col[(size_t)e * A.ld];
        arg = x > mx ? e : arg;
        mx = x > mx ? x : mx;
    }
    float total = 0.f;
    for (int e = 0; e < A.m; ++e)
        total += fast_exp(col[(size_t)e * A.ld] - mx);
    if (A.logp != nullptr)
        A.logp[item] = (fast_log(total) + mx) - fast_log((float)A.m);
    if (A.member == nullptr) return;
    int chosen = arg;
    if (A.mode == 0) {
        // sample_from_likelihoods (random.hpp:316-333) as written
        uint32_t xs = lcg_mulmod(A.seed_batch, A.pow_lo[item & 4095]);
        xs = lcg_mulmod(xs, A.pow_hi[item >> 12]);
        float t = total * lcg_unif01(xs);
        chosen = A.m - 1;
        for (int e = 0; e < A.m; ++e) {
            t -= fast_exp(col[(size_t)e * A.ld] - mx);
            if (t <= 0.f) {
                chosen = e;
                break;
            }
        }
    }
    A.member[item] = (uint32_t)chosen;
    if (A.group != nullptr)
        A.group[item] = A.groups[(size_t)chosen * A.groups_ld + item];
}

// the most rows of one workgroup's chunk (its list may hold them all)
constexpr int kPickMaxRows = 8192;
// the chunk of a workgroup: the expected list, rows / m, fills a wave
constexpr int predict_many_pick_rows(size_t m) {
    return m * 64 < (size_t)kPickMaxRows ? (int)(m * 64) : kPickMaxRows;
}
// dynamic LDS of k_predict_many_pick: the list
constexpr size_t predict_many_pick_lds(int rows) { return (size_t)rows * 4; }

// Phase B: the group in the chosen member only.  Workgroup (chunk, member e)
// compacts the chunk's rows with member[q] == e into its list by ballot, then
// runs k_predict's passes with a lane per listed row.  Grid (chunks, M).
template <int KIND0, int KIND1, int NF>
__global__ __launch_bounds__(kBlock) void k_predict_many_pick(
        const PredictMember * __restrict__ all,
        const uint32_t * __restrict__ member, int rows) {
    extern __shared__ uint32_t pm_list[];
    __shared__ uint32_t s_exp[1024];
    __shared__ unsigned s_count;
    if (threadIdx.x == 0) s_count = 0;
    predict_load_exp(s_exp);
    const PredictMember & M = all[blockIdx.y];
    const size_t n_rows = M.P.row_end;
    const size_t r0 = (size_t)blockIdx.x * (size_t)rows;
    const size_t r1 = r0 + (size_t)rows < n_rows ? r0 + (size_t)rows : n_rows;
    const unsigned lane = threadIdx.x & 63u;
    for (size_t q0 = r0 + (threadIdx.x & ~63u); q0 < r1; q0 += kBlock) {
        const size_t q = q0 + lane;
        const bool mine = q < r1 && member[q] == blockIdx.y;
        const unsigned long long mask = __ballot(mine);
        if (mask == 0) continue;
        unsigned at = 0;
        if (lane == 0) at = atomicAdd(&s_count, (unsigned)__popcll(mask));
        at = __shfl(at, 0);
        if (mine)
            pm_list[at + __popcll(mask & ((1ull << lane) - 1ull))] =
                (uint32_t)q;
    }
    __syncthreads();
    const unsigned count = s_count;
    if (count == 0) return;
    const SweepParams & P = M.P;
    const PredictArgs & A = M.B;
#define PREDICT_COUNT count
#define PREDICT_FIRST threadIdx.x
#define PREDICT_STRIDE kBlock
#define PREDICT_ROW(item) pm_list[item]
#define PREDICT_LOGP(x) x
#include "kernels_predict_body.h"
#undef PREDICT_COUNT
#undef PREDICT_FIRST
#undef PREDICT_STRIDE
#undef PREDICT_ROW
#undef PREDICT_LOGP
}

}  // namespace dist
