// Held-out rows: draw whole rows and missing cells from the mixture
// (DESIGN.md 4.12).  Part of kernels.h.
//
// Per query row q with mask observed[q] (bit f: feature f of the row is
// observed; null: nothing is):
//   scores[k] = driver score_value (k_predict_prior), then in feature order
//               (mixture.hpp:416-425) every OBSERVED feature's accumulate with
//               the row's value; an unobserved feature contributes nothing
//               (the fold predict_feature calls `base`);
//   group[q]  = sample_from_scores_overwrite (random.hpp:361-366) with engine
//               step draw_base + q + 1 of seed_state (batch_row_unif01), as a
//               global id: predict's draw when everything is observed;
//   cell(q,f) = for every feature that is not observed, sample_cell_word
//               (sample.h) on the drawn group's statistics, keyed by
//               (seed_state, draw_base + q, f); an observed cell is copied.
// One launch: a lane per row draws its group and then its cells; the loop
// over the features is uniform, so a wave is in one kind at a time.
//
// With no mask at all every row scores the driver's vector alone: its
// likelihoods exp(prior[k] - max) and their in-order total are then the same
// for every row.  k_sample_prior_lik forms them once per call (one exponential
// per group) and k_sample_rows<true> leaves each row its subtractive scan over
// them, k wave-uniform, by scalar loads.  The floats are those the generic
// instance forms per row, in the same order.
#pragma once

#include "sample.h"

namespace dist {

struct SampleArgs {
    const float * prior;        // [K] the driver's score_value
    const float * lik;          // [K + 1]: exp(prior[k] - max), then the total
                                // (the nothing-observed instance)
    const uint32_t * observed;  // [rows of the launch] or null: none observed
    const uint32_t * p2g;       // packed slot -> global id
    uint32_t * out[kMaxF];      // [rows of the launch]; may be P.values[f]
    uint32_t * group;           // [rows of the launch] or null
    const float * w[kMaxF];     // DD: alphas; DPD: betas (sample.h)
    uint32_t seed_state;
    unsigned long long row0;    // draw_base + the launch's first query
    unsigned long long q0;      // the launch's first query
    // [0]: min over (query << 8 | feature) of the observed values outside
    // their domain; [1]: of the cells whose bounded loop ran out
    unsigned long long * bad;
};

// likelihoods of the driver's scores alone (scores_to_likelihoods,
// random.cc:94-106) and their in-order total: one thread, K exponentials
__global__ void k_sample_prior_lik(int K, const float * __restrict__ prior,
                                   float * __restrict__ lik) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const float ea = u2f(g_tables_dev.exp_ab[0]);
    const float eb = u2f(g_tables_dev.exp_ab[1]);
    float m = prior[0];
    for (int k = 1; k < K; ++k) m = prior[k] > m ? prior[k] : m;
    float total = 0.f;
    for (int k = 0; k < K; ++k) {
        const float l =
            fast_exp_nonpos(prior[k] - m, g_tables_dev.exp_table, ea, eb);
        lik[k] = l;
        total += l;
    }
    lik[K] = total;
}

// One lane's query row under its mask; at(k) is its score against slot k
// (FeatureScorer's shape without a target: k wave-uniform, per-group entries
// by scalar loads, a per-lane gather only for a categorical table).
struct SampleScorer {
    const SweepParams & P;
    const float * prior;
    uint32_t ob;
    uint32_t x[kMaxF];
    float lf[kMaxF];

    __device__ __forceinline__ SampleScorer(const SweepParams & P_,
                                            const SampleArgs & A, size_t q,
                                            uint32_t ob_)
        : P(P_), prior(A.prior), ob(ob_) {
        for (int f = 0; f < P.F; ++f) {
            const int kind = P.feat[f].kind;
            const uint32_t dim = (uint32_t)P.feat[f].dim;
            uint32_t v = 0u;
            // words in unobserved cells are never read
            if ((ob >> f) & 1u) {
                v = P.values[f][q];
                // dd.hpp:125 and bb.hpp assert these in debug builds; here
                // they would index outside the tables
                const bool bad = (kind == DIST_DD && v >= dim)
                                 || (kind == DIST_BB && v > 1u);
                if (bad) {
                    atomicMin(A.bad, ((A.q0 + q) << 8) | (unsigned)f);
                    v = 0u;
                }
                // dpd.hpp:534-542: a value the table does not hold is OTHER
                if (kind == DIST_DPD && v >= dim) v = DIST_DPD_OTHER;
            }
            x[f] = v;
            lf[f] = kind == DIST_GP ? fast_log_factorial(v) : 0.f;
        }
    }
    __device__ __forceinline__ Entry entry_at(const SlaveView & v, int kind,
                                              int k, uint32_t xv) const {
        Entry e;
        e.c0 = as_uniform(v.c0)[k];
        if (is_cat(kind)) {
            e.c1 = (kind == DIST_DPD && xv == DIST_DPD_OTHER)
                       ? v.other
                       : v.S[(size_t)xv * v.cap + k];
            e.c2 = 0.f;
            e.c3 = 0.f;
        } else {
            e.c1 = as_uniform(v.c1)[k];
            e.c2 = as_uniform(v.c2)[k];
            e.c3 = as_uniform(v.c3)[k];
        }
        return e;
    }
    __device__ __forceinline__ float at(int k) const {
        float s = as_uniform(prior)[k];
        for (int f = 0; f < P.F; ++f) {
            if (!((ob >> f) & 1u)) continue;
            const int kind = P.feat[f].kind;
            s = accumulate(kind, s, entry_at(P.feat[f], kind, k, x[f]), x[f],
                           lf[f], P.feat[f].p);
        }
        return s;
    }
};

// UNCOND: no mask was given, the likelihoods are A.lik.  P.values are the
// launch's query columns (null where no row observes the feature),
// P.row_begin = 0, P.row_end the launch's row count, P.seed_batch the engine
// state one step before the launch's first row's draw.  The loop over the
// rows is kernels_sample_body.h, shared with k_sample_rows_pick
// (kernels_sample_many.h).
template <bool UNCOND>
__global__ __launch_bounds__(kBlock) void k_sample_rows(SweepParams P,
                                                        SampleArgs A) {
    __shared__ uint32_t s_exp[1024];
    if (!UNCOND) {
        for (int i = threadIdx.x; i < 1024; i += kBlock)
            s_exp[i] = g_tables_dev.exp_table[i];
        __syncthreads();
    }
#define SAMPLE_COUNT P.row_end
#define SAMPLE_FIRST (size_t)blockIdx.x * kBlock + threadIdx.x
#define SAMPLE_STRIDE (size_t)gridDim.x * kBlock
#define SAMPLE_ROW(item) item
#include "kernels_sample_body.h"
#undef SAMPLE_COUNT
#undef SAMPLE_FIRST
#undef SAMPLE_STRIDE
#undef SAMPLE_ROW
}

}  // namespace dist
