// Held-out rows: one feature's predictive given the others.
// Part of kernels.h.
//
// Per query row q, target feature t, candidate words cand[0..C) for t and a
// bit mask observed[q] (bit f: feature f of the row is observed; bit t is
// ignored):
//   scores_c[k] = driver score_value (k_predict_prior), then in feature order
//                 (mixture.hpp:416-425) every OBSERVED feature's accumulate
//                 with the row's value and, at position t, the target's with
//                 cand[c]; an unobserved feature contributes nothing;
//   joint[q][c] = log_sum_exp(scores_c) (random.cc:78-92);
//   base[q]     = log_sum_exp of the same fold with the target left out;
//   choice[q]   = an index into cand: sample_from_scores_overwrite
//                 (random.hpp:361-366) over joint[q][0..C) with engine step
//                 draw_base + q + 1 of seed_state, or the first maximum.
// Everything but the target's term is the same for all candidates of a row:
// k_predict_feature evaluates it once per (row, group, pass) into LDS and the
// C + 1 chains of the row (the candidates and `base`) read it from there.
// k_predict_feature_recompute is the plain form, a lane per (row, slot)
// scoring its completed row as PredictScorer does: the A/B partner and an
// independent witness of the staged form.
#pragma once

namespace dist {

struct FeatureArgs {
    const float * prior;        // [K] the driver's score_value
    const uint32_t * observed;  // [rows of the launch] or null: all observed
    const uint32_t * cand;      // [C] candidate words, validated by the host
                                // (a DPD word outside the table is OTHER)
    int target;
    int C;                      // 0: only `base` is wanted
    int items;                  // staged form: (row, slot) items a workgroup takes
    int rows;                   // ... and the most rows they can touch
    int tile;                   // ... groups per LDS tile
    float * joint;              // [rows of the launch][C] or null
    float * base;               // [rows of the launch] or null
    // the launch's first query, counted from the call's first
    unsigned long long q0;
    // min over (query << 8 | feature) of the observed values outside their
    // domain
    unsigned long long * bad;
};

// the most rows one workgroup of k_predict_feature stages
constexpr int kFeatureRowsMax = 32;

// dynamic LDS of k_predict_feature: one plane of prefix scores and one plane
// per additive term after the target, each [rows][tile + 1] floats (the odd
// row stride keeps the rows of a wave in different banks)
constexpr size_t predict_feature_lds(int terms_after, int tile, int rows) {
    return (size_t)(1 + terms_after) * (size_t)(tile + 1) * (size_t)rows * 4;
}

// The term `accumulate` adds for the kinds whose fold is acc + term (BB, GP,
// BNB, NICH): the very expression inside accumulate's parentheses, which
// score_group spells.  -ffp-contract=off and IEEE evaluation make
// acc + feature_term(...) the bits of accumulate(acc, ...).  The categorical
// kinds fold as (acc + c1) - c0 and stage both floats.
DIST_HD float feature_term(int kind, const Entry & e, uint32_t value, float lf,
                           const float * p) {
    return score_group(kind, e, value, lf, p);
}

// a query row's word of feature `kind` as the scorers take it, or the bad
// word's report (PredictScorer's rules)
__device__ __forceinline__ uint32_t feature_query_word(
        const FeatureArgs & A, int kind, uint32_t dim, uint32_t v, size_t q,
        int f) {
    // dd.hpp:125 and bb.hpp assert these in debug builds; here they would
    // index outside the tables
    const bool bad = (kind == DIST_DD && v >= dim)
                     || (kind == DIST_BB && v > 1u);
    if (bad) {
        atomicMin(A.bad, ((A.q0 + q) << 8) | (unsigned)f);
        v = 0u;
    }
    // dpd.hpp:534-542: a value the table does not hold is OTHER
    if (kind == DIST_DPD && v >= dim) v = DIST_DPD_OTHER;
    return v;
}

// the target's accumulate for candidate word cw at group k (k wave-uniform:
// the per-group entry by scalar loads, a per-lane gather for a table).  TK is
// the target's kind; DIST_DD also serves DPD, with the OTHER test.
template <int TK>
__device__ __forceinline__ float feature_target(const SlaveView & tv, float s,
                                                int k, uint32_t cw, float lf,
                                                bool other) {
    Entry e;
    e.c0 = as_uniform(tv.c0)[k];
    if (TK == DIST_DD) {
        e.c1 = other ? tv.other : tv.S[(size_t)cw * tv.cap + k];
        e.c2 = 0.f;
        e.c3 = 0.f;
    } else {
        e.c1 = as_uniform(tv.c1)[k];
        e.c2 = as_uniform(tv.c2)[k];
        e.c3 = as_uniform(tv.c3)[k];
    }
    return accumulate(TK, s, e, cw, lf, tv.p);
}

// The staged form.  Work items are (row, slot) pairs, slot in [0, C] (slot C
// is the row's `base` chain), numbered row-major over the launch; a workgroup
// takes A.items consecutive ones, which touch at most A.rows rows.  Per pass
// (maximum, then sum) and per tile of A.tile groups:
//   staging   threads over (row, k): prefix[row][k] = the driver score folded
//             with the observed features before t, and the additive terms of
//             every observed feature after t (one float, or c1 and c0 for a
//             categorical feature);
//   chains    a lane per item walks the tile's k in order: prefix (an LDS
//             read that is the same for all lanes of a row), the target's
//             accumulate with its own candidate, the after-terms in order,
//             then the maximum or the exponential's sum.
// Chain state is carried across tiles.  P.values are the launch's query
// columns (the target's may be null), P.row_end the launch's row count.
template <int TK>
__global__ __launch_bounds__(kBlock) void k_predict_feature(SweepParams P,
                                                            FeatureArgs A) {
#define FEATURE_OUT(x) x
#include "kernels_feature_body.h"
#undef FEATURE_OUT
}

// The plain form: a lane per (row, slot) folds its completed row group by
// group, as PredictScorer::at does, skipping what is not observed.  Kinds at
// run time.
struct FeatureScorer {
    const SweepParams & P;
    const float * prior;
    uint32_t ob;          // observed features, bit t: the slot has a candidate
    uint32_t x[kMaxF];
    float lf[kMaxF];

    __device__ __forceinline__ FeatureScorer(const SweepParams & P_,
                                             const FeatureArgs & A, size_t q,
                                             int slot)
        : P(P_), prior(A.prior) {
        const int t = A.target;
        ob = (A.observed ? A.observed[q] : ~0u) & ~(1u << t);
        for (int f = 0; f < P.F; ++f) {
            const int kind = P.feat[f].kind;
            uint32_t v = 0u;
            if ((ob >> f) & 1u)
                v = feature_query_word(A, kind, (uint32_t)P.feat[f].dim,
                                       P.values[f][q], q, f);
            if (f == t && slot < A.C) {
                v = A.cand[slot];
                ob |= 1u << t;
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

__global__ __launch_bounds__(kBlock) void k_predict_feature_recompute(
        SweepParams P, FeatureArgs A) {
    __shared__ uint32_t s_exp[1024];
    for (int i = threadIdx.x; i < 1024; i += kBlock)
        s_exp[i] = g_tables_dev.exp_table[i];
    __syncthreads();
    const float ea = u2f(g_tables_dev.exp_ab[0]);
    const float eb = u2f(g_tables_dev.exp_ab[1]);
    const int K = P.K;
    const size_t S = (size_t)A.C + 1;
    const size_t n_items = (size_t)P.row_end * S;
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t item = (size_t)blockIdx.x * kBlock + threadIdx.x;
         item < n_items; item += stride) {
        const size_t q = item / S;
        const int slot = (int)(item - q * S);
        const FeatureScorer fs(P, A, q, slot);
        float m = fs.at(0);
        for (int k = 1; k < K; ++k) {
            const float s = fs.at(k);
            m = s > m ? s : m;
        }
        float total = 0.f;
        for (int k = 0; k < K; ++k)
            total += fast_exp_nonpos(fs.at(k) - m, s_exp, ea, eb);
        const float out = fast_log(total) + m;
        if (slot < A.C) {
            if (A.joint != nullptr) A.joint[q * (size_t)A.C + slot] = out;
        } else if (A.base != nullptr) {
            A.base[q] = out;
        }
    }
}

// choice[q] over joint[q][0..C), which is read only: mode 1 the first index
// of maximal joint; mode 0 sample_from_scores_overwrite (scores_to_likelihoods,
// random.cc:94-106; sample_from_likelihoods, random.hpp:316-333) with the
// row's own engine step (batch_row_unif01).  A lane per row.
__global__ void k_predict_feature_choice(SweepParams P,
                                         const float * __restrict__ joint,
                                         int C, int mode,
                                         uint32_t * __restrict__ choice) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= P.row_end) return;
    const float ea = u2f(g_tables_dev.exp_ab[0]);
    const float eb = u2f(g_tables_dev.exp_ab[1]);
    const float * j = joint + q * (size_t)C;
    float m = j[0];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
        const float s = j[c];
        arg = s > m ? c : arg;
        m = s > m ? s : m;
    }
    int pick = arg;
    if (mode == 0) {
        float total = 0.f;
        for (int c = 0; c < C; ++c)
            total += fast_exp_nonpos(j[c] - m, g_tables_dev.exp_table, ea, eb);
        float t = total * batch_row_unif01(P, q);
        pick = C - 1;
        for (int c = 0; c < C; ++c) {
            t -= fast_exp_nonpos(j[c] - m, g_tables_dev.exp_table, ea, eb);
            if (t <= 0.f) {
                pick = c;
                break;
            }
        }
    }
    choice[q] = (uint32_t)pick;
}

// One feature's predictive against M engines at once: per
// member e the planes
//   wj[e][q * C + c] = k_predict_feature's joint on member e, bit for bit;
//                      under LowEntropy minus the member's prior total, one
//                      float subtraction (predict_minus);
//   wb[e][q]         = the same for base;
// which k_ensemble_fold folds over the members into joint and base (and the
// member drawn from wb), and k_predict_feature_choice reads the folded joint.
// One member of the call, read from a device array by blockIdx.y as
// PredictMember is: A.joint and A.base point into the member's planes.
struct FeatureMember {
    SweepParams P;
    FeatureArgs A;
    float * prior;       // [K] = A.prior, as k_predict_prior_many writes it
    float * total;       // the member's prior total, or null (not wanted)
    const float * sub;   // = total under LowEntropy, else null
};

// Phase A: k_predict_feature's staged form for every (member, item); grid
// (item blocks, M).  The member is workgroup-uniform, so are its parameters
// and the scalar loads of feature_target.  items, rows, tile and the LDS size
// are the same in every member (the host takes the tile from the largest K of
// the call): a member of fewer groups ends its tile loop early.
template <int TK>
__global__ __launch_bounds__(kBlock) void k_predict_feature_many(
        const FeatureMember * __restrict__ all) {
    const FeatureMember & M = all[blockIdx.y];
    const SweepParams & P = M.P;
    const FeatureArgs & A = M.A;
    const float * const sub = M.sub;
#define FEATURE_OUT(x) predict_minus(x, sub)
#include "kernels_feature_body.h"
#undef FEATURE_OUT
}

}  // namespace dist
