// The body k_predict shares with the ensemble's kernels (kernels_ensemble.h),
// included INSIDE each of them.  It is text and not a __device__ function on
// purpose: moved into a function, force-inlined and otherwise verbatim, it
// compiled to other code in every k_predict instance (another register
// allocation; a scratch copy of the parameters in the GP + NICH one), and
// k_predict is to stay the code it was.
//
// The including function provides
//   P, A       a SweepParams and a PredictArgs (objects or references),
//              KIND0, KIND1, NF, and the LDS copy s_exp[1024] of the
//              exponential's table, loaded and synchronised;
//   PREDICT_COUNT         the number of rows it walks,
//   PREDICT_FIRST, PREDICT_STRIDE   a lane's first item and step: whole waves
//              iterate together,
//   PREDICT_ROW(item)     the item's row in the launch,
//   PREDICT_LOGP(x)       what is written for a row whose log_sum_exp is x.
//
// One lane = one query row, groups in index order: 64 independent in-order
// chains per wave, as in k_sweep_sample.  Scores are recomputed per pass.
    const float ea = u2f(g_tables_dev.exp_ab[0]);
    const float eb = u2f(g_tables_dev.exp_ab[1]);
    const int K = P.K;
    const bool draw = A.group != nullptr && A.mode == 0;

    const size_t stride = PREDICT_STRIDE;
    const size_t n = PREDICT_COUNT;
    // whole waves iterate together so that the vote below sees every lane
    const size_t n_round = (n + 63) / 64 * 64;
    for (size_t item = PREDICT_FIRST; item < n_round; item += stride) {
        const bool live = item < n;
        const size_t q = live ? PREDICT_ROW(item) : 0;
        const PredictScorer<KIND0, KIND1, NF> ps(P, A, q, live);
        // vector_max (vector_math.cc:74-83); the first index that attains it
        float m = ps.at(0);
        int arg = 0;
#pragma unroll kSweepUnroll
        for (int k = 1; k < K; ++k) {
            const float s = ps.at(k);
            arg = s > m ? k : arg;
            m = s > m ? s : m;
        }
        int g2 = arg;
        if (A.logp != nullptr || draw) {
            float total = 0.f;
#pragma unroll kSweepUnroll
            for (int k = 0; k < K; ++k)
                total += fast_exp_nonpos(ps.at(k) - m, s_exp, ea, eb);
            if (live && A.logp != nullptr)
                A.logp[q] = PREDICT_LOGP(fast_log(total) + m);
            if (draw) {
                // sample_from_likelihoods: the first index with t <= 0 is
                // the number of steps after which t is still positive
                float t = total * batch_row_unif01(P, q);
                int steps = 0;
                for (int k0 = 0; k0 < K; k0 += kSweepUnroll) {
#pragma unroll
                    for (int j = 0; j < kSweepUnroll; ++j) {
                        const int k = k0 + j;
                        if (k < K) {
                            t -= fast_exp_nonpos(ps.at(k) - m, s_exp, ea, eb);
                            steps += t > 0.f ? 1 : 0;
                        }
                    }
                    if (!__any(live && t > 0.f)) break;
                }
                g2 = steps < K - 1 ? steps : K - 1;
            }
        }
        if (live && A.group != nullptr) A.group[q] = A.p2g[g2];
    }
