// The engine's hyper-parameter step (dist_gibbs_score_data_grid,
// dist_gibbs_score_counts_grid, dist_gibbs_sample_*): score_data_grid of
// mixture.hpp:433-438 / dd.hpp:259-284 with DirichletDiscrete's work following
// what changed between candidates, PitmanYor::score_counts
// (clustering.cc:152-183) for a grid of (alpha, d), and
// sample_from_scores_overwrite (random.hpp:361-392) without the scores leaving
// the device.  Part of kernels.h.
#pragma once

namespace dist {

// ---------------------------------------------------------------------------
// DirichletDiscrete.  A candidate's score is vector_sum over dim + 1
// accumulators (dd.hpp:287-318): accumulator v < dim is a function of
// alphas[v] alone, the last one ("shift") of alpha_sum alone.  The host lists
// every DISTINCT accumulator of a grid once -- a job -- and says per candidate
// which jobs make up its dim + 1 values.
//
// MixtureDataScorer::_init skips groups without members, _update (the
// incremental form, dd.hpp:259-284) walks all of them.  The terms they differ
// by are, for an empty group, fast_lgamma(a + 0.f) - fast_lgamma(a) and
// fast_lgamma(alpha_sum) - fast_lgamma(alpha_sum + 0.f): a + 0.f == a for
// every float a, fast_lgamma is a pure function, and x - x == +0 for every
// finite x; an accumulator that starts at +0 and only ever has such sums
// added never holds -0, so adding +0 leaves its bits alone.  Skipping the
// empty groups therefore gives _update's value bit for bit.

struct HyperJob {
    float a;   // alphas[v], or alpha_sum for the shift accumulator
    int v;     // coordinate, or dim: the shift accumulator
};

// One lane per job walks the K groups in index order (the reference's float
// accumulation order).  Lanes of a wave take adjacent jobs; the host orders
// the jobs so that those are adjacent coordinates wherever it can, and
// cnt[k][v .. v + 63] is then one coalesced read per group.  The shift jobs
// come last and read i0[k] uniformly.
__global__ __launch_bounds__(64) void k_hyper_dd_chains(
        SlaveView s, const HyperJob * __restrict__ jobs, int n_jobs,
        float * __restrict__ vals) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= n_jobs) return;
    const float a = jobs[j].a;
    const int v = jobs[j].v;
    const float shared_part = fast_lgamma(a);
    float acc = 0.f;
    if (v < s.dim) {
        for (int k = 0; k < s.K; ++k)
            if (s.i0[k])
                acc += fast_lgamma(a + (float)s.cnt[(size_t)k * s.dim + v])
                     - shared_part;
    } else {
        for (int k = 0; k < s.K; ++k)
            if (s.i0[k])
                acc += shared_part - fast_lgamma(a + (float)s.i0[k]);
    }
    vals[j] = acc;
}

// The closing pass: candidate c's accumulators are vals[pick[c][0 .. dim]];
// vector_sum in the association of vector_sum_as_built (models.h), read
// through the index list instead of from an array.
__global__ void k_hyper_dd_close(const int * __restrict__ pick,
                                 const float * __restrict__ vals, int width,
                                 int n, float * __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const int * mine = pick + (size_t)c * width;
    float sum = 0.f;
    if (width < 4) {
        for (int i = 0; i < width; ++i) sum += vals[mine[i]];
    } else {
        float l0 = 0.f, l1 = 0.f, l2 = 0.f, l3 = 0.f;
        const int body = width & ~3;
        for (int i = 0; i < body; i += 4) {
            l0 += vals[mine[i]];
            l1 += vals[mine[i + 1]];
            l2 += vals[mine[i + 2]];
            l3 += vals[mine[i + 3]];
        }
        sum = (l1 + l3) + (l0 + l2);
        for (int i = body; i < width; ++i) sum += vals[mine[i]];
    }
    out[c] = sum;
}

// DirichletProcessDiscrete's grid is summed in binary64 (k_score_data_grid);
// the scores the draw reads are floats
__global__ void k_hyper_narrow(const double * __restrict__ in, int n,
                               float * __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}

// ---------------------------------------------------------------------------
// PitmanYor::score_counts for a grid of (alpha, d): before[] -- the non-empty
// groups and rows ahead of every group -- is formed once for all candidates;
// blockIdx.x = candidate.  The terms are summed in binary64 like
// k_py_score_counts, here in a fixed order (every lane its strided groups,
// the wave by shuffles, the waves in index order), so that replicas with
// equal statistics get equal scores.
constexpr int kHyperCountsBlock = 256;
__global__ __launch_bounds__(kHyperCountsBlock) void k_hyper_py_grid(
        const int32_t * __restrict__ counts,
        const unsigned long long * __restrict__ before, int K,
        const float * __restrict__ alphas, const float * __restrict__ ds,
        float * __restrict__ out) {
    __shared__ double wave_sum[kHyperCountsBlock / 64];
    const int c = blockIdx.x;
    const float alpha = alphas[c], d = ds[c];
    double acc = 0.0;
    for (int k = threadIdx.x; k < K; k += kHyperCountsBlock)
        if (counts[k] > 0)
            acc += py_score_counts_term(alpha, d, counts[k], before[2 * k],
                                        before[2 * k + 1]);
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int w = 0; w < kHyperCountsBlock / 64; ++w) total += wave_sum[w];
        out[c] = (float)total;
    }
}

// ---------------------------------------------------------------------------
// sample_from_scores_overwrite (random.hpp:361-392) over the n scores of a
// grid, with one engine step from rng_state: the index and the advanced state
// go to pinned host memory, the scores stay where they are.
struct HyperDraw {
    uint32_t index;
    uint32_t rng_state;
};
__global__ void k_hyper_draw(float * __restrict__ scores, int n,
                             uint32_t rng_state, HyperDraw * pinned_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    rng_state = lcg_mulmod(rng_state, 16807u);
    SampleOut out;
    sample_scalar(1, n, scores, 0.f, lcg_unif01(rng_state), &out);
    pinned_out->index = (uint32_t)out.sample;
    pinned_out->rng_state = rng_state;
}

}  // namespace dist
