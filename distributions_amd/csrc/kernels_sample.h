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
// state one step before the launch's first row's draw.
template <bool UNCOND>
__global__ __launch_bounds__(kBlock) void k_sample_rows(SweepParams P,
                                                        SampleArgs A) {
    __shared__ uint32_t s_exp[1024];
    if (!UNCOND) {
        for (int i = threadIdx.x; i < 1024; i += kBlock)
            s_exp[i] = g_tables_dev.exp_table[i];
        __syncthreads();
    }
    const float ea = u2f(g_tables_dev.exp_ab[0]);
    const float eb = u2f(g_tables_dev.exp_ab[1]);
    const int K = P.K, F = P.F;
    const uint32_t fmask = F >= 32 ? ~0u : (1u << F) - 1u;
    uint32_t nullmask = 0u;
    for (int f = 0; f < F; ++f)
        nullmask |= P.values[f] == nullptr ? 1u << f : 0u;

    const size_t stride = (size_t)gridDim.x * kBlock;
    const size_t n = P.row_end;
    // whole waves iterate together so that the votes below see every lane
    const size_t n_round = (n + 63) / 64 * 64;
    for (size_t item = (size_t)blockIdx.x * kBlock + threadIdx.x;
         item < n_round; item += stride) {
        const bool live = item < n;
        const size_t q = live ? item : 0;
        uint32_t ob = (UNCOND || !live) ? 0u : (A.observed[q] & fmask);
        // a feature without a column is one no row observes
        if (ob & nullmask) {
            atomicMin(A.bad,
                      ((A.q0 + q) << 8) | (unsigned)(__ffs(ob & nullmask) - 1));
            ob &= ~nullmask;
        }

        // ---- the group --------------------------------------------------
        int g2;
        if (UNCOND) {
            // sample_from_likelihoods over the call's one likelihood vector
            float t = as_uniform(A.lik)[K] * batch_row_unif01(P, q);
            int steps = 0;
            for (int k0 = 0; k0 < K; k0 += kSweepUnroll) {
#pragma unroll
                for (int j = 0; j < kSweepUnroll; ++j) {
                    const int k = k0 + j;
                    if (k < K) {
                        t -= as_uniform(A.lik)[k];
                        steps += t > 0.f ? 1 : 0;
                    }
                }
                if (!__any(live && t > 0.f)) break;
            }
            g2 = steps < K - 1 ? steps : K - 1;
        } else {
            const SampleScorer sc(P, A, q, ob);
            // vector_max (vector_math.cc:74-83)
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
            // sample_from_likelihoods: the first index with t <= 0 is the
            // number of steps after which t is still positive
            float t = total * batch_row_unif01(P, q);
            int steps = 0;
            for (int k0 = 0; k0 < K; k0 += kSweepUnroll) {
#pragma unroll
                for (int j = 0; j < kSweepUnroll; ++j) {
                    const int k = k0 + j;
                    if (k < K) {
                        t -= fast_exp_nonpos(sc.at(k) - m, s_exp, ea, eb);
                        steps += t > 0.f ? 1 : 0;
                    }
                }
                if (!__any(live && t > 0.f)) break;
            }
            g2 = steps < K - 1 ? steps : K - 1;
        }
        if (live && A.group != nullptr) A.group[q] = A.p2g[g2];

        // ---- the cells --------------------------------------------------
        for (int f = 0; f < F; ++f) {
            if (!live) continue;
            const SlaveView & v = P.feat[f];
            uint32_t * out = A.out[f];
            if ((ob >> f) & 1u) {
                // an observed cell comes back as given (in place: untouched)
                if (out != P.values[f]) out[q] = P.values[f][q];
                continue;
            }
            SampleShared sh;
            sh.kind = v.kind;
            sh.dim = v.dim;
            sh.p[0] = v.p[0]; sh.p[1] = v.p[1];
            sh.p[2] = v.p[2]; sh.p[3] = v.p[3];
            sh.w = A.w[f];
            // the drawn group's statistics, by its packed index
            const Stats st = {v.i0[g2], v.i1[g2], v.f0[g2], v.f1[g2]};
            const int32_t * cnt =
                is_cat(v.kind) ? v.cnt + (size_t)g2 * v.dim : nullptr;
            bool exhausted = false;
            out[q] = sample_cell_word(v.kind, sh, st, cnt, A.seed_state,
                                      A.row0 + q, f, &exhausted);
            if (exhausted)
                atomicMin(A.bad + 1, ((A.q0 + q) << 8) | (unsigned)f);
        }
    }
}

}  // namespace dist
