// Held-out rows: log marginals of S feature subsets per row over M engines,
// and the moments mutual information is estimated from.
// Part of kernels.h.
//
// Per query row q, mask masks[s] (bit f: feature f is observed; the masks are
// shared by all rows) and member e:
//   scores[k]  = driver score_value (k_predict_prior), then in feature order
//                (mixture.hpp:416-425) the accumulate of every feature NAMED
//                by masks[s] with the row's value; an unnamed feature
//                contributes nothing;
//   w[e][q][s] = log_sum_exp(scores) (random.cc:78-92); under LowEntropy
//                minus the member's prior total (predict_minus);
// the fold k_predict_feature calls `base`, with the mask per chain instead of
// per row.  Every additive term is the same in all S chains of a row:
// k_marginals_many stages the terms of the features in the union of the masks
// once per (row, group, pass) and the chains differ only in which they keep.
// k_ensemble_fold folds the planes over the members.
#pragma once

namespace dist {

struct MarginalsArgs {
    const float * prior;        // [K] the driver's score_value
    const uint32_t * masks;     // [S], validated by the host: no bit >= F
    int S;
    uint32_t named;             // the union of the masks
    int items;                  // (row, mask) items a workgroup takes
    int rows;                   // ... and the most rows they can touch
    int tile;                   // ... groups per LDS tile
    float * out;                // [rows of the launch][S]
    // the launch's first query, counted from the call's first
    unsigned long long q0;
    // min over (query << 8 | feature) of the named values outside their
    // domain
    unsigned long long * bad;
};

// One member of the call, read from a device array by blockIdx.y as
// FeatureMember is: A.out points into the member's plane.
struct MarginalsMember {
    SweepParams P;
    MarginalsArgs A;
    float * prior;       // [K] = A.prior, as k_predict_prior_many writes it
    float * total;       // the member's prior total, or null (not wanted)
    const float * sub;   // = total under LowEntropy, else null
};

// the most rows one workgroup of k_marginals_many stages (with one mask a row
// is one item: more rows than k_predict_feature takes keep a wave of chains)
constexpr int kMarginalsRowsMax = 64;

// dynamic LDS of k_marginals_many: the plane of driver scores and one plane
// per additive term of the named features (one for BB, GP, BNB and NICH; c1
// and c0 for DD and DPD), each [rows][tile + 1] floats as
// predict_feature_lds lays them out: the case "target before feature 0"
constexpr size_t marginals_lds(int terms, int tile, int rows) {
    return predict_feature_lds(terms, tile, rows);
}

// a query row's word of feature `kind` as the scorers take it, or the bad
// word's report (feature_query_word's rules)
__device__ __forceinline__ uint32_t marginals_query_word(
        const MarginalsArgs & A, int kind, uint32_t dim, uint32_t v, size_t q,
        int f) {
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

// Work items are (row, mask) pairs numbered row-major over the launch, which
// is their index into the member's plane; a workgroup takes A.items
// consecutive ones, which touch at most A.rows rows (a row of more than
// kBlock masks spans workgroups).  Per pass (maximum, then sum) and per tile
// of A.tile groups:
//   staging   threads over (row, k): the driver score and, per named feature,
//             its additive term at the row's value (feature_term, or c1 and
//             c0 of a categorical feature);
//   chains    a lane per item walks the tile's k in order: s = prior, then
//             per named feature u = s + term (or (s + c1) - c0) and
//             s = bit_f(mask) ? u : s -- accumulate's operations where the
//             bit is set and nothing where it is not, without divergence --
//             then the maximum or the exponential's sum.
// Chain state is carried across tiles.  Grid (item blocks, M): the member is
// workgroup-uniform.  items, rows, tile and the LDS size are the same in every
// member (the host takes the tile from the largest K of the call): a member
// of fewer groups ends its tile loop early.
__global__ __launch_bounds__(kBlock) void k_marginals_many(
        const MarginalsMember * __restrict__ all) {
    extern __shared__ float mg_lds[];
    __shared__ uint32_t s_exp[1024];
    __shared__ uint32_t s_x[kMarginalsRowsMax][kMaxF];
    __shared__ float s_lf[kMarginalsRowsMax][kMaxF];
    const MarginalsMember & M = all[blockIdx.y];
    const SweepParams & P = M.P;
    const MarginalsArgs & A = M.A;
    const float * const sub = M.sub;
    const int tid = threadIdx.x;
    for (int i = tid; i < 1024; i += kBlock)
        s_exp[i] = g_tables_dev.exp_table[i];
    const float ea = u2f(g_tables_dev.exp_ab[0]);
    const float eb = u2f(g_tables_dev.exp_ab[1]);
    const int K = P.K, F = P.F;
    const size_t n = P.row_end;
    const size_t S = (size_t)A.S;
    const size_t n_items = n * S;
    const size_t item0 = (size_t)blockIdx.x * (size_t)A.items;
    if (item0 >= n_items) return;
    const size_t item1 = min(n_items, item0 + (size_t)A.items);
    const size_t q_lo = item0 / S;
    // rows this workgroup touches (<= A.rows by the host's choice of items)
    const int R = (int)((item1 - 1) / S - q_lo) + 1;
    const int T = A.tile, Tp = T + 1;
    const size_t plane = (size_t)A.rows * Tp;
    const uint32_t named = A.named;

    uint32_t catmask = 0;
    for (int f = 0; f < F; ++f)
        catmask |= is_cat(P.feat[f].kind) ? 1u << f : 0u;
    // the rows' words of the named features (the others are never read)
    for (int f = 0; f < F; ++f) {
        if (!((named >> f) & 1u)) continue;
        const int kind = P.feat[f].kind;
        const uint32_t dim = (uint32_t)P.feat[f].dim;
        if (tid < R) {
            const uint32_t v = marginals_query_word(
                A, kind, dim, P.values[f][q_lo + tid], q_lo + tid, f);
            s_x[tid][f] = v;
            s_lf[tid][f] = kind == DIST_GP ? fast_log_factorial(v) : 0.f;
        }
    }

    // this lane's item: its row's planes and its mask, read once
    const size_t item = item0 + tid;
    const bool lane_on = tid < A.items && item < item1;
    const size_t q = lane_on ? item / S : q_lo;
    const uint32_t mask = lane_on ? A.masks[item - q * S] : 0u;
    const float * pre = mg_lds + (size_t)(q - q_lo) * Tp;

    float m = 0.f, total = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
        for (int k0 = 0; k0 < K; k0 += T) {
            const int tn = min(T, K - k0);
            __syncthreads();   // the words; the last tile's readers are done
            for (int i = tid; i < R * tn; i += kBlock) {
                const int r = i / tn, kk = i - r * tn, k = k0 + kk;
                float * dst = mg_lds + (size_t)r * Tp + kk;
                dst[0] = A.prior[k];
                int pl = 1;
                for (int f = 0; f < F; ++f) {
                    if (!((named >> f) & 1u)) continue;
                    const SlaveView & v = P.feat[f];
                    const uint32_t x = s_x[r][f];
                    const Entry e = load_entry(v, k, x);
                    if ((catmask >> f) & 1u) {
                        dst[(size_t)pl * plane] = e.c1;
                        dst[(size_t)(pl + 1) * plane] = e.c0;
                        pl += 2;
                    } else {
                        dst[(size_t)pl * plane] =
                            feature_term(v.kind, e, x, s_lf[r][f], v.p);
                        pl += 1;
                    }
                }
            }
            __syncthreads();
            for (int kk = 0; kk < tn; ++kk) {
                float s = pre[kk];
                int pl = 1;
                for (int f = 0; f < F; ++f) {
                    if (!((named >> f) & 1u)) continue;
                    float u;
                    if ((catmask >> f) & 1u) {
                        u = (s + pre[(size_t)pl * plane + kk])
                            - pre[(size_t)(pl + 1) * plane + kk];
                        pl += 2;
                    } else {
                        u = s + pre[(size_t)pl * plane + kk];
                        pl += 1;
                    }
                    s = (mask >> f) & 1u ? u : s;
                }
                // vector_max (vector_math.cc:74-83), then the in-order sum
                if (pass == 0) m = (k0 + kk == 0 || s > m) ? s : m;
                else total += fast_exp_nonpos(s - m, s_exp, ea, eb);
            }
        }
    }
    if (lane_on) A.out[item] = predict_minus(fast_log(total) + m, sub);
}

// The plain form for ONE mask: a row then has one chain and staging shares
// nothing, so a lane per row folds the named features group by group from the
// engines' tables, as PredictScorer does for a whole row; the mask is the
// wave's, so skipping an unnamed feature is a scalar branch.  The host
// launches this form for S == 1 and the staged form from two masks on.  A
// mask that names EVERY feature takes the loop without the per-feature test
// (PredictScorer::at as it is): the test inside the k loop keeps the compiler
// from unrolling it over k, 5.2 ms against 1.66 ms at DD-256, M = 8, 10^5 rows.
// KIND0, KIND1, NF: k_predict's instances (Gibbs::dispatch).
template <int KIND0, int KIND1, int NF>
struct MarginalsScorer {
    static constexpr int kUnroll = NF > 0 ? NF : 1;
    const SweepParams & P;
    const float * prior;
    uint32_t mask;
    uint32_t x[kMaxF];
    float lf[kMaxF];

    __device__ __forceinline__ int nf() const { return NF > 0 ? NF : P.F; }
    __device__ __forceinline__ int kind_of(int f) const {
        if (f == 0 && KIND0 >= 0) return KIND0;
        if (f == 1 && KIND1 >= 0) return KIND1;
        return P.feat[f].kind;
    }
    __device__ __forceinline__ MarginalsScorer(const SweepParams & P_,
                                               const MarginalsArgs & A,
                                               size_t q, uint32_t mask_)
        : P(P_), prior(A.prior), mask(mask_) {
#pragma unroll kUnroll
        for (int f = 0; f < nf(); ++f) {
            const int kind = kind_of(f);
            uint32_t v = 0u;
            // words of unnamed features are never read
            if ((mask >> f) & 1u)
                v = marginals_query_word(A, kind, (uint32_t)P.feat[f].dim,
                                         P.values[f][q], q, f);
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
    // ALL: the mask names every feature and nothing is tested in the loop
    // (the same floats: every test would pass)
    template <bool ALL>
    __device__ __forceinline__ float at(int k) const {
        float s = as_uniform(prior)[k];
#pragma unroll kUnroll
        for (int f = 0; f < nf(); ++f) {
            if (!ALL && !((mask >> f) & 1u)) continue;
            const int kind = kind_of(f);
            s = accumulate(kind, s, entry_at(P.feat[f], kind, k, x[f]), x[f],
                           lf[f], P.feat[f].p);
        }
        return s;
    }
};

// log_sum_exp of a row's scores: vector_max (vector_math.cc:74-83), then the
// in-order sum
template <bool ALL, class Scorer>
__device__ __forceinline__ float marginals_lse(const Scorer & ms, int K,
                                               const uint32_t * s_exp,
                                               float ea, float eb) {
    float m = ms.template at<ALL>(0);
#pragma unroll kSweepUnroll
    for (int k = 1; k < K; ++k) {
        const float s = ms.template at<ALL>(k);
        m = s > m ? s : m;
    }
    float total = 0.f;
#pragma unroll kSweepUnroll
    for (int k = 0; k < K; ++k)
        total += fast_exp_nonpos(ms.template at<ALL>(k) - m, s_exp, ea, eb);
    return fast_log(total) + m;
}

template <int KIND0, int KIND1, int NF>
__global__ __launch_bounds__(kBlock) void k_marginals_plain(
        const MarginalsMember * __restrict__ all) {
    __shared__ uint32_t s_exp[1024];
    predict_load_exp(s_exp);
    const MarginalsMember & M = all[blockIdx.y];
    const SweepParams & P = M.P;
    const MarginalsArgs & A = M.A;
    const float * const sub = M.sub;
    const float ea = u2f(g_tables_dev.exp_ab[0]);
    const float eb = u2f(g_tables_dev.exp_ab[1]);
    const int K = P.K;
    const size_t n_items = P.row_end;      // (S == 1: an item is a row)
    const uint32_t mask = __builtin_amdgcn_readfirstlane(A.masks[0]);
    const uint32_t every = (1u << (NF > 0 ? NF : P.F)) - 1u;
    const bool whole = (mask & every) == every;
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t item = (size_t)blockIdx.x * kBlock + threadIdx.x;
         item < n_items; item += stride) {
        const MarginalsScorer<KIND0, KIND1, NF> ms(P, A, item, mask);
        const float lse = whole ? marginals_lse<true>(ms, K, s_exp, ea, eb)
                                : marginals_lse<false>(ms, K, s_exp, ea, eb);
        A.out[item] = predict_minus(lse, sub);
    }
}

// The moments of the mutual-information estimate.  L is the
// folded plane of one chunk of n drawn rows, [n][S] with S = F + F (F - 1) / 2:
// column i < F the log marginal of feature i alone, then the pairs (i, j),
// i < j, in row-major order.  With
//   d_q = (double)L_ij[q] - (double)L_i[q] - (double)L_j[q]   (i < j)
//   d_q = -(double)L_i[q]                                      (i == j)
// cell c = i * F + j (i <= j) of acc = [F * F][3] doubles accumulates
// sum_q (d_q - shift) and sum_q (d_q - shift)^2 and keeps shift, the d of the
// call's first row: the sums of d and d^2 follow from them exactly enough
// (relate_many), and the variance does not cancel where |mean| is many
// standard deviations, as an entropy's is.  One workgroup per cell and no
// floating-point atomics: lane t sums the rows t, t + kBlock, ... in order,
// an LDS tree in fixed order adds the lanes, and thread 0 adds the chunk's
// sums to acc -- chunks follow each other in stream order, so a call's bits
// do not depend on when it runs.  first: the call's first chunk.
__global__ __launch_bounds__(kBlock) void k_relate_moments(
        const float * __restrict__ L, size_t n, int F, int first,
        double * acc) {
    __shared__ double s_a[kBlock];
    __shared__ double s_b[kBlock];
    const int i = blockIdx.x / F, j = blockIdx.x - i * F;
    if (i > j) return;
    const size_t S = (size_t)F + (size_t)F * (F - 1) / 2;
    // the pair's column: pairs of i come after those of 0 .. i - 1
    const size_t cij =
        (size_t)F + (size_t)i * F - (size_t)i * (i + 1) / 2 + (j - i - 1);
    double * const cell = acc + 3 * (size_t)blockIdx.x;
    const double shift = first
        ? (i == j ? -(double)L[i]
                  : (double)L[cij] - (double)L[i] - (double)L[j])
        : cell[2];
    double a = 0.0, b = 0.0;
    for (size_t q = threadIdx.x; q < n; q += kBlock) {
        const float * row = L + q * S;
        const double d = i == j
            ? -(double)row[i]
            : (double)row[cij] - (double)row[i] - (double)row[j];
        // (a row whose marginals are not finite makes the cell NaN)
        const double dd = isfinite(d) ? d - shift : (double)NAN;
        a += dd;
        b += dd * dd;
    }
    s_a[threadIdx.x] = a;
    s_b[threadIdx.x] = b;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            s_a[threadIdx.x] += s_a[threadIdx.x + w];
            s_b[threadIdx.x] += s_b[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        cell[0] += s_a[0];
        cell[1] += s_b[0];
        if (first) cell[2] = shift;
    }
}

}  // namespace dist
