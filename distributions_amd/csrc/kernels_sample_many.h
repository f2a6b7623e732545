// Whole rows and missing cells drawn from an ensemble of M engines
// (DESIGN.md 4.16).  Part of kernels.h.
//
// Per query row q with mask observed[q] (null: nothing is observed) and member
// e (an engine: one posterior sample of the partition and the
// hyper-parameters):
//   wb[e][q]  = log_sum_exp (random.cc:78-92) of k_sample_rows' scores of row
//               q on member e: the driver's score_value folded with every
//               OBSERVED feature's accumulate, the fold predict_feature calls
//               `base`; under LowEntropy minus the member's prior total;
//   base[q]   = log_sum_exp(wb[0..M)[q]) - fast_log((float)M);
//   member[q] = sample_from_scores_overwrite (random.hpp:361-366) over
//               wb[.][q] with engine step draw_base + q + 1 of the member
//               stream (k_ensemble_fold);
//   group[q], cell(q, f) = k_sample_rows' on member member[q]: the group with
//               engine step draw_base + q + 1 of seed_state, the cells keyed
//               by (seed_state, draw_base + q, f).
// Phase A (k_sample_base_many) writes the planes wb, k_ensemble_fold folds
// them, phase B (k_sample_rows_pick) draws group and cells in the chosen
// member only.  With no mask wb[e][.] is one number per member:
// k_sample_prior_lik_many forms it with the member's likelihoods and fills
// the plane, and no phase A runs.
#pragma once

namespace dist {

// One member of the call, read from a device array by blockIdx.y (as
// PredictMember and FeatureMember): everything k_sample_rows takes as kernel
// arguments.
struct SampleMember {
    SweepParams P;
    SampleArgs A;        // A.prior and A.lik are the member's own
    float * lik;         // [K + 1] = A.lik, as k_sample_prior_lik_many writes it
    float * wb;          // the member's plane: [rows of the launch], or with
                         // no mask [fill] (every row the same number)
    const float * sub;   // the member's prior total under LowEntropy, else null
};

// Phase A: wb[e][q] for every (member, row); grid (row blocks, M), a lane per
// row.  The member is wave-uniform, so are its parameters and the scalar
// loads of SampleScorer::at.  The floats are k_predict_feature's `base`: the
// maximum, the in-order sum of the exponentials, fast_log(total) + max.
__global__ __launch_bounds__(kBlock) void k_sample_base_many(
        const SampleMember * __restrict__ all) {
    __shared__ uint32_t s_exp[1024];
    predict_load_exp(s_exp);
    const SampleMember & M = all[blockIdx.y];
    const SweepParams & P = M.P;
    const SampleArgs & A = M.A;
    const float ea = u2f(g_tables_dev.exp_ab[0]);
    const float eb = u2f(g_tables_dev.exp_ab[1]);
    const int K = P.K, F = P.F;
    const uint32_t fmask = F >= 32 ? ~0u : (1u << F) - 1u;
    uint32_t nullmask = 0u;
    for (int f = 0; f < F; ++f)
        nullmask |= P.values[f] == nullptr ? 1u << f : 0u;
    const size_t n = P.row_end;
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t q = (size_t)blockIdx.x * kBlock + threadIdx.x; q < n;
         q += stride) {
        uint32_t ob = A.observed[q] & fmask;
        // a feature without a column is one no row observes
        if (ob & nullmask) {
            atomicMin(A.bad,
                      ((A.q0 + q) << 8) | (unsigned)(__ffs(ob & nullmask) - 1));
            ob &= ~nullmask;
        }
        const SampleScorer sc(P, A, q, ob);
        // vector_max (vector_math.cc:74-83), then the in-order sum
        float m = sc.at(0);
#pragma unroll kSweepUnroll
        for (int k = 1; k < K; ++k) {
            const float s = sc.at(k);
            m = s > m ? s : m;
        }
        float total = 0.f;
#pragma unroll kSweepUnroll
        for (int k = 0; k < K; ++k)
            total += fast_exp_nonpos(sc.at(k) - m, s_exp, ea, eb);
        M.wb[q] = predict_minus(fast_log(total) + m, M.sub);
    }
}

// k_sample_prior_lik for every member in one launch, a workgroup per member:
// the K exponentials go over the workgroup's lanes, the maximum and the
// in-order total are taken by one lane in index order, so the floats are
// k_sample_prior_lik's.  The workgroup then fills the member's plane with the
// one number every row of a call without a mask has for it: fast_log(total) +
// max (minus the prior total under LowEntropy), the zero mask's wb.
__global__ __launch_bounds__(kBlock) void k_sample_prior_lik_many(
        const SampleMember * __restrict__ all, size_t fill) {
    __shared__ float s_m;
    const SampleMember & M = all[blockIdx.x];
    const int K = M.P.K;
    const float * prior = M.A.prior;
    float * lik = M.lik;
    const float ea = u2f(g_tables_dev.exp_ab[0]);
    const float eb = u2f(g_tables_dev.exp_ab[1]);
    if (threadIdx.x == 0) {
        float m = prior[0];
        for (int k = 1; k < K; ++k) m = prior[k] > m ? prior[k] : m;
        s_m = m;
    }
    __syncthreads();
    const float m = s_m;
    for (int k = threadIdx.x; k < K; k += kBlock)
        lik[k] = fast_exp_nonpos(prior[k] - m, g_tables_dev.exp_table, ea, eb);
    __syncthreads();   // (the workgroup's own global stores, then its loads)
    if (threadIdx.x == 0) {
        float total = 0.f;
        for (int k = 0; k < K; ++k) total += lik[k];
        lik[K] = total;
        s_m = predict_minus(fast_log(total) + m, M.sub);
    }
    __syncthreads();
    if (M.wb == nullptr) return;
    const float wb = s_m;
    for (size_t q = threadIdx.x; q < fill; q += kBlock) M.wb[q] = wb;
}

// Phase B: group and cells in the chosen member only.  Workgroup (chunk,
// member e) compacts the chunk's rows with member[q] == e into its list by
// ballot, exactly as k_predict_many_pick does (the chunk is
// predict_many_pick_rows(M), the list predict_many_pick_lds of it), then runs
// k_sample_rows' body with a lane per listed row: the member's parameters are
// workgroup-uniform, so the per-group entries still come by scalar loads.
// Every row is written by exactly one workgroup, so completion in place is
// safe.  Grid (chunks, M).
template <bool UNCOND>
__global__ __launch_bounds__(kBlock) void k_sample_rows_pick(
        const SampleMember * __restrict__ all,
        const uint32_t * __restrict__ member, int rows) {
    extern __shared__ uint32_t sm_list[];
    __shared__ uint32_t s_exp[1024];
    __shared__ unsigned s_count;
    if (threadIdx.x == 0) s_count = 0;
    if (!UNCOND) {
        for (int i = threadIdx.x; i < 1024; i += kBlock)
            s_exp[i] = g_tables_dev.exp_table[i];
    }
    __syncthreads();
    const SampleMember & M = all[blockIdx.y];
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
            sm_list[at + __popcll(mask & ((1ull << lane) - 1ull))] =
                (uint32_t)q;
    }
    __syncthreads();
    const unsigned count = s_count;
    // a member nobody of the chunk drew
    if (count == 0) return;
    const SweepParams & P = M.P;
    const SampleArgs & A = M.A;
#define SAMPLE_COUNT count
#define SAMPLE_FIRST threadIdx.x
#define SAMPLE_STRIDE kBlock
#define SAMPLE_ROW(item) sm_list[item]
#include "kernels_sample_body.h"
#undef SAMPLE_COUNT
#undef SAMPLE_FIRST
#undef SAMPLE_STRIDE
#undef SAMPLE_ROW
}

}  // namespace dist
