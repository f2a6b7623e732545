// The body k_predict_feature shares with k_predict_feature_many, included
// INSIDE each of them: text and not a __device__ function, for the reason
// kernels_predict_body.h gives (k_predict_feature is to stay the code it was).
//
// The including function provides
//   P, A       a SweepParams and a FeatureArgs (objects or references), TK,
//   FEATURE_OUT(x)   what is written for an item whose log_sum_exp is x.
//
// Work items are (row, slot) pairs; see k_predict_feature's comment.
    extern __shared__ float pf_lds[];
    __shared__ uint32_t s_exp[1024];
    __shared__ uint32_t s_x[kFeatureRowsMax][kMaxF];
    __shared__ float s_lf[kFeatureRowsMax][kMaxF];
    __shared__ uint32_t s_obs[kFeatureRowsMax];
    const int tid = threadIdx.x;
    for (int i = tid; i < 1024; i += kBlock)
        s_exp[i] = g_tables_dev.exp_table[i];
    const float ea = u2f(g_tables_dev.exp_ab[0]);
    const float eb = u2f(g_tables_dev.exp_ab[1]);
    const int K = P.K, F = P.F, t = A.target;
    const size_t n = P.row_end;
    const size_t S = (size_t)A.C + 1;
    const size_t n_items = n * S;
    const size_t item0 = (size_t)blockIdx.x * (size_t)A.items;
    const size_t item1 = min(n_items, item0 + (size_t)A.items);
    const size_t q_lo = item0 / S;
    // rows this workgroup touches (<= A.rows by the host's choice of items)
    const int R = (int)((item1 - 1) / S - q_lo) + 1;
    const int T = A.tile, Tp = T + 1;
    const size_t plane = (size_t)A.rows * Tp;

    // the rows' masks and observed words
    uint32_t catmask = 0;
    for (int f = 0; f < F; ++f)
        catmask |= is_cat(P.feat[f].kind) ? 1u << f : 0u;
    if (tid < R) {
        const uint32_t ob = A.observed ? A.observed[q_lo + tid] : ~0u;
        s_obs[tid] = ob & ~(1u << t);
    }
    __syncthreads();
    for (int f = 0; f < F; ++f) {
        const int kind = P.feat[f].kind;
        const uint32_t dim = (uint32_t)P.feat[f].dim;
        if (tid < R) {
            uint32_t v = 0u;
            float lf = 0.f;
            // words in unobserved cells are never read
            if ((s_obs[tid] >> f) & 1u) {
                v = feature_query_word(A, kind, dim, P.values[f][q_lo + tid],
                                       q_lo + tid, f);
                lf = kind == DIST_GP ? fast_log_factorial(v) : 0.f;
            }
            s_x[tid][f] = v;
            s_lf[tid][f] = lf;
        }
    }
    __syncthreads();

    // this lane's item
    const size_t item = item0 + tid;
    const bool lane_on = tid < A.items && item < item1;
    const size_t q = lane_on ? item / S : q_lo;
    const int slot = lane_on ? (int)(item - q * S) : A.C;
    const int r_l = (int)(q - q_lo);
    const bool is_cand = lane_on && slot < A.C;
    const uint32_t ob = lane_on ? s_obs[r_l] : 0u;
    const SlaveView & tv = P.feat[t];
    const uint32_t cw = is_cand ? A.cand[slot] : 0u;
    // (a lane without a candidate evaluates the target's term as well and
    // drops it: no divergence in the chain; it gathers nothing out of a DPD
    // table, which may be empty)
    const bool other = tv.kind == DIST_DPD
                       && (!is_cand || cw == DIST_DPD_OTHER);
    const float lf_c = TK == DIST_GP ? fast_log_factorial(cw) : 0.f;
    const float * pre = pf_lds + (size_t)r_l * Tp;

    float m = 0.f, total = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
        for (int k0 = 0; k0 < K; k0 += T) {
            const int tn = min(T, K - k0);
            __syncthreads();   // the last tile's readers are done
            for (int i = tid; i < R * tn; i += kBlock) {
                const int r = i / tn, kk = i - r * tn, k = k0 + kk;
                const uint32_t obr = s_obs[r];
                float * dst = pf_lds + (size_t)r * Tp + kk;
                float s = A.prior[k];
                int pl = 1;
                for (int f = 0; f < F; ++f) {
                    if (f == t) {
                        dst[0] = s;
                        continue;
                    }
                    const SlaveView & v = P.feat[f];
                    const bool on = (obr >> f) & 1u;
                    const bool cat = (catmask >> f) & 1u;
                    if (f > t) pl += cat ? 2 : 1;
                    if (!on) continue;
                    const uint32_t x = s_x[r][f];
                    const Entry e = load_entry(v, k, x);
                    if (f < t) {
                        s = accumulate(v.kind, s, e, x, s_lf[r][f], v.p);
                    } else if (cat) {
                        dst[(size_t)(pl - 2) * plane] = e.c1;
                        dst[(size_t)(pl - 1) * plane] = e.c0;
                    } else {
                        dst[(size_t)(pl - 1) * plane] =
                            feature_term(v.kind, e, x, s_lf[r][f], v.p);
                    }
                }
            }
            __syncthreads();
            if (t + 1 == F) {   // nothing after the target: the tight loop
#pragma unroll 4
                for (int kk = 0; kk < tn; ++kk) {
                    const int k = k0 + kk;
                    float s = pre[kk];
                    const float u =
                        feature_target<TK>(tv, s, k, cw, lf_c, other);
                    s = is_cand ? u : s;
                    if (pass == 0) m = (k == 0 || s > m) ? s : m;
                    else total += fast_exp_nonpos(s - m, s_exp, ea, eb);
                }
                continue;
            }
            for (int kk = 0; kk < tn; ++kk) {
                const int k = k0 + kk;
                float s = pre[kk];
                const float ut = feature_target<TK>(tv, s, k, cw, lf_c, other);
                s = is_cand ? ut : s;
                int pl = 1;
                for (int f = t + 1; f < F; ++f) {
                    const bool on = (ob >> f) & 1u;
                    float u;
                    if ((catmask >> f) & 1u) {
                        u = (s + pre[(size_t)pl * plane + kk])
                            - pre[(size_t)(pl + 1) * plane + kk];
                        pl += 2;
                    } else {
                        u = s + pre[(size_t)pl * plane + kk];
                        pl += 1;
                    }
                    s = on ? u : s;
                }
                // vector_max (vector_math.cc:74-83), then the in-order sum
                if (pass == 0) m = (k == 0 || s > m) ? s : m;
                else total += fast_exp_nonpos(s - m, s_exp, ea, eb);
            }
        }
    }
    if (lane_on) {
        const float out = FEATURE_OUT(fast_log(total) + m);
        if (is_cand) {
            if (A.joint != nullptr) A.joint[q * (size_t)A.C + slot] = out;
        } else if (A.base != nullptr) {
            A.base[q] = out;
        }
    }
