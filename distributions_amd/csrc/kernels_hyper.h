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
// (one accumulator: coordinate v < dim under alphas[v] = a, or the shift
// accumulator under alpha_sum = a)
__device__ __forceinline__ float hyper_dd_chain(
        int K, int dim, const int32_t * __restrict__ i0,
        const int32_t * __restrict__ cnt, float a, int v) {
    const float shared_part = fast_lgamma(a);
    float acc = 0.f;
    if (v < dim) {
        for (int k = 0; k < K; ++k)
            if (i0[k])
                acc += fast_lgamma(a + (float)cnt[(size_t)k * dim + v])
                     - shared_part;
    } else {
        for (int k = 0; k < K; ++k)
            if (i0[k])
                acc += shared_part - fast_lgamma(a + (float)i0[k]);
    }
    return acc;
}
__global__ __launch_bounds__(64) void k_hyper_dd_chains(
        SlaveView s, const HyperJob * __restrict__ jobs, int n_jobs,
        float * __restrict__ vals) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= n_jobs) return;
    vals[j] = hyper_dd_chain(s.K, s.dim, s.i0, s.cnt, jobs[j].a, jobs[j].v);
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

// ---------------------------------------------------------------------------
// A whole coordinate pass of a DirichletDiscrete feature
// (dist_gibbs_sample_hypers_pass): n_coords steps of "grid over
// alphas[coords[i]], draw, install" without the host in between.
//
// Phase 1, k_hyper_dd_chains_many: the accumulator of coordinate u depends on
// alphas[u] alone, so every chain of the whole pass runs before the first
// draw -- per engine the dim alphas in force (jobs 0 .. dim-1), then the
// grid's distinct (coordinate, value) pairs, which all engines share.
// Phase 2, k_hyper_dd_pass: what depends on the draws -- alpha_sum and the
// shift accumulator under it, the closing vector_sum, the draw -- in one
// resident workgroup per engine.
struct HyperPassEngine {
    int K, dim;
    const int32_t * i0;    // group sizes
    const int32_t * cnt;   // [K][dim]
    const float * alphas;  // the alphas in force (Slave::prior)
    float * vals;          // [dim + n_grid_jobs]: phase 1's accumulators
    uint32_t * out;        // [n_coords + 1]: chosen[], the advanced rng state
    uint32_t rng_state;
};

// blockIdx.y = engine, as k_predict_many and k_chains pick theirs
__global__ __launch_bounds__(64) void k_hyper_dd_chains_many(
        const HyperPassEngine * __restrict__ engines,
        const HyperJob * __restrict__ grid_jobs, int n_grid_jobs) {
    const HyperPassEngine & e = engines[blockIdx.y];
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int dim = e.dim;
    if (j >= dim + n_grid_jobs) return;
    const float a = j < dim ? e.alphas[j] : grid_jobs[j - dim].a;
    const int v = j < dim ? j : grid_jobs[j - dim].v;
    e.vals[j] = hyper_dd_chain(e.K, dim, e.i0, e.cnt, a, v);
}

constexpr int kHyperPassBlock = 1024;
// a lane per candidate closes and sums: G <= the block
constexpr int kHyperPassMaxGrid = kHyperPassBlock;
// LDS floats for one chunk of shift terms ([groups of the chunk][G]); K is
// walked in chunks of kHyperPassTerms / G groups, so it is not bounded
constexpr int kHyperPassTerms = 8192;

static inline size_t k_hyper_dd_pass_lds(int G, int chunk) {
    const size_t Gp = ((size_t)G + 3) & ~(size_t)3;
    return sizeof(float) * (2 * DIST_DD_MAX_DIM + 3 * Gp + (size_t)chunk * G);
}

// grid[i * grid_stride + c]: step i's values (grid_stride 0: one grid for
// every step); grid_job[i * G + c]: where phase 1 left the accumulator of
// (coords[i], that value) in vals[].  Every loop is bounded by n_coords, G,
// K or dim; the workgroup meets at __syncthreads() only.
__global__ __launch_bounds__(kHyperPassBlock) void k_hyper_dd_pass(
        const HyperPassEngine * __restrict__ engines,
        const int * __restrict__ coords, int n_coords,
        const float * __restrict__ grid, int G, int grid_stride,
        const int * __restrict__ grid_job, int chunk) {
    extern __shared__ __attribute__((aligned(16))) char hyper_pass_lds[];
    const int Gp = (G + 3) & ~3;
    float * alphas = (float *)hyper_pass_lds;   // in force, as drawn so far
    float * acc = alphas + DIST_DD_MAX_DIM;     // their accumulators
    float * csum = acc + DIST_DD_MAX_DIM;       // the step's alpha_sums
    float * lg_s = csum + Gp;                   // fast_lgamma of them
    float * scores = lg_s + Gp;
    float * terms = scores + Gp;                // [chunk][G]

    const HyperPassEngine & e = engines[blockIdx.x];
    const int dim = e.dim, K = e.K;
    const int32_t * __restrict__ i0 = e.i0;
    const float * __restrict__ vals = e.vals;
    const int t = threadIdx.x;
    for (int u = t; u < dim; u += kHyperPassBlock) {
        alphas[u] = e.alphas[u];
        acc[u] = vals[u];
    }
    uint32_t state = e.rng_state;
    // thread t's first (group, candidate) of a chunk and its stride
    const int dk = kHyperPassBlock / G, dc = kHyperPassBlock % G;
    const int k_first = t / G, c_first = t - k_first * G;
    __syncthreads();

    for (int i = 0; i < n_coords; ++i) {
        const int v = coords[i];
        const float * __restrict__ g = grid + (size_t)i * grid_stride;
        if (t == 0) {
            // candidate 0: _init's float sum in index order; then _update's
            // binary64 carry over the one coordinate that changes
            float a = 0.f;
            for (int u = 0; u < dim; ++u) a += u == v ? g[0] : alphas[u];
            double alpha_sum_d = a;
            csum[0] = (float)alpha_sum_d;
            for (int c = 1; c < G; ++c) {
                if (g[c] != g[c - 1])
                    alpha_sum_d += (double)g[c] - (double)g[c - 1];
                csum[c] = (float)alpha_sum_d;
            }
        }
        __syncthreads();
        if (t < G) lg_s[t] = fast_lgamma(csum[t]);
        __syncthreads();
        // the shift accumulator of candidate t, groups in index order.  A
        // group without members contributes +0 here and is skipped by
        // k_hyper_dd_chains: the sum starts at +0 and never holds -0, so the
        // bits agree (see the top of this file).
        float shift = 0.f;
        for (int k0 = 0; k0 < K; k0 += chunk) {
            const int kn = K - k0 < chunk ? K - k0 : chunk;
            int k = k_first, c = c_first;
            while (k < kn) {
                const int n = i0[k0 + k];
                terms[k * G + c] =
                    n ? lg_s[c] - fast_lgamma(csum[c] + (float)n) : 0.f;
                k += dk;
                c += dc;
                if (c >= G) {
                    c -= G;
                    k += 1;
                }
            }
            __syncthreads();
            if (t < G) {
#pragma unroll 8
                for (int kk = 0; kk < kn; ++kk) shift += terms[kk * G + t];
            }
            __syncthreads();
        }
        if (t < G) {
            // vector_sum_as_built over the dim + 1 accumulators: position v
            // from the candidate's chain, position dim the shift sum
            const float mine = vals[grid_job[(size_t)i * G + t]];
            const int width = dim + 1;
            auto x = [&](int p) {
                return p == v ? mine : (p == dim ? shift : acc[p]);
            };
            float sum = 0.f;
            if (width < 4) {
                for (int p = 0; p < width; ++p) sum += x(p);
            } else {
                float l0 = 0.f, l1 = 0.f, l2 = 0.f, l3 = 0.f;
                const int body = width & ~3;
                for (int p = 0; p < body; p += 4) {
                    l0 += x(p);
                    l1 += x(p + 1);
                    l2 += x(p + 2);
                    l3 += x(p + 3);
                }
                sum = (l1 + l3) + (l0 + l2);
                for (int p = body; p < width; ++p) sum += x(p);
            }
            scores[t] = sum;
        }
        __syncthreads();
        if (t == 0) {
            state = lcg_mulmod(state, 16807u);
            SampleOut out;
            sample_scalar(1, G, scores, 0.f, lcg_unif01(state), &out);
            alphas[v] = g[out.sample];
            acc[v] = vals[grid_job[(size_t)i * G + out.sample]];
            e.out[i] = (uint32_t)out.sample;
        }
        __syncthreads();
    }
    if (t == 0) e.out[n_coords] = state;
}

}  // namespace dist
