// Held-out rows: log predictive density and group draw of rows that are NOT
// in the table, against the engine's current state.  Part of
// kernels.h.
//
// Per query row q with values x_q[f]:
//   scores[k] = driver score_value (clustering.hpp:195-208, or the generic
//               MixtureDriver score under LowEntropy, mixture.hpp:124-141)
//               + every slave's score_value in feature order
//               (mixture.hpp:416-425), k in [0, K), empty groups included;
//   logp[q]   = log_sum_exp(scores) (random.cc:78-92): max, the in-order sum
//               of fast_exp(scores[k] - max), fast_log(total) + max;
//   group[q]  = sample_from_scores_overwrite (random.hpp:361-366,
//               random.cc:94-106, random.hpp:316-333) with engine step
//               draw_base + q + 1 of seed_state, or the first argmax; as a
//               global id.
// The arithmetic per (row, group) is that of k_score_rows; nothing n x K is
// ever stored.
#pragma once

namespace dist {

struct PredictArgs {
    const float * prior;       // [K] the driver's score_value (k_predict_prior)
    const uint32_t * p2g;      // packed slot -> global id
    float * logp;              // [rows of the launch] or null
    uint32_t * group;          // [rows of the launch] or null
    int mode;                  // 0: draw, 1: first argmax
    // the launch's first query, counted from the call's first
    unsigned long long q0;
    // min over (query << 8 | feature) of the values outside their domain
    unsigned long long * bad;
};

// MixtureDriver::score_value, the same expressions as k_score_rows: the
// scores do not depend on the row, so they are formed once per call
__global__ void k_predict_prior(SweepParams P, float * __restrict__ prior) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P.K) return;
    prior[k] = P.cluster == 1
        ? le_score_add_value(P.dataset_size, P.counts[k], (int)P.sample_size,
                             P.n_empty)
        : P.shifted[k] + P.scalars->shift_full;
}

// One lane's query row; at(k) is its score against slot k (k wave-uniform:
// per-group parameters by scalar loads, a per-lane gather only for a
// categorical table).  Template arguments as RowScorer's.
template <int KIND0, int KIND1, int NF>
struct PredictScorer {
    static constexpr int kUnroll = NF > 0 ? NF : 1;
    const SweepParams & P;
    const float * prior;
    uint32_t x[kMaxF];
    float lf[kMaxF];

    __device__ __forceinline__ int nf() const { return NF > 0 ? NF : P.F; }
    __device__ __forceinline__ int kind_of(int f) const {
        if (f == 0 && KIND0 >= 0) return KIND0;
        if (f == 1 && KIND1 >= 0) return KIND1;
        return P.feat[f].kind;
    }

    // live = false: a padding lane of the last wave, which scores zeros
    __device__ __forceinline__ PredictScorer(const SweepParams & P_,
                                             const PredictArgs & A, size_t q,
                                             bool live)
        : P(P_), prior(A.prior) {
#pragma unroll kUnroll
        for (int f = 0; f < nf(); ++f) {
            const int kind = kind_of(f);
            uint32_t v = live ? P.values[f][q] : 0u;
            const uint32_t dim = (uint32_t)P.feat[f].dim;
            // dd.hpp:125 and bb.hpp assert these in debug builds; here they
            // would index outside the tables
            const bool bad = (kind == DIST_DD && v >= dim)
                             || (kind == DIST_BB && v > 1u);
            if (bad) {
                atomicMin(A.bad, ((A.q0 + q) << 8) | (unsigned)f);
                v = 0u;
            }
            // dpd.hpp:534-542: a value the table does not hold is OTHER
            if (kind == DIST_DPD && v >= dim) v = DIST_DPD_OTHER;
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
#pragma unroll kUnroll
        for (int f = 0; f < nf(); ++f) {
            const int kind = kind_of(f);
            s = accumulate(kind, s, entry_at(P.feat[f], kind, k, x[f]), x[f],
                           lf[f], P.feat[f].p);
        }
        return s;
    }
};

// One lane = one query row; the body, shared with kernels_ensemble.h, is
// kernels_predict_body.h.  P.values are the launch's query columns,
// P.row_begin = 0, P.row_end the launch's row count, P.seed_batch the engine
// state one step before the launch's first row's draw.
template <int KIND0, int KIND1, int NF>
__global__ __launch_bounds__(kBlock) void k_predict(SweepParams P,
                                                    PredictArgs A) {
    __shared__ uint32_t s_exp[1024];
    for (int i = threadIdx.x; i < 1024; i += kBlock)
        s_exp[i] = g_tables_dev.exp_table[i];
    __syncthreads();
#define PREDICT_COUNT P.row_end
#define PREDICT_FIRST (size_t)blockIdx.x * kBlock + threadIdx.x
#define PREDICT_STRIDE (size_t)gridDim.x * kBlock
#define PREDICT_ROW(item) item
#define PREDICT_LOGP(x) x
#include "kernels_predict_body.h"
#undef PREDICT_COUNT
#undef PREDICT_FIRST
#undef PREDICT_STRIDE
#undef PREDICT_ROW
#undef PREDICT_LOGP
}

}  // namespace dist
