// The body k_sample_rows shares with k_sample_rows_pick, included INSIDE each
// of them: text and not a __device__ function, for the reason
// kernels_predict_body.h gives (k_sample_rows is to stay the code it was).
//
// The including function provides
//   P, A       a SweepParams and a SampleArgs (objects or references), UNCOND,
//   s_exp      the LDS copy of the exponential's table (loaded if !UNCOND),
//   SAMPLE_COUNT              the number of work items,
//   SAMPLE_FIRST, SAMPLE_STRIDE   this lane's first item and its step,
//   SAMPLE_ROW(item)          the row of the launch that item stands for.
// Whole waves iterate together (the count is rounded up with dead lanes), so
// that the votes below see every lane: SAMPLE_FIRST and SAMPLE_STRIDE must
// keep the lanes of a wave on 64 consecutive items.
    const float ea = u2f(g_tables_dev.exp_ab[0]);
    const float eb = u2f(g_tables_dev.exp_ab[1]);
    const int K = P.K, F = P.F;
    const uint32_t fmask = F >= 32 ? ~0u : (1u << F) - 1u;
    uint32_t nullmask = 0u;
    for (int f = 0; f < F; ++f)
        nullmask |= P.values[f] == nullptr ? 1u << f : 0u;

    const size_t stride = SAMPLE_STRIDE;
    const size_t n = SAMPLE_COUNT;
    // whole waves iterate together so that the votes below see every lane
    const size_t n_round = (n + 63) / 64 * 64;
    for (size_t item = SAMPLE_FIRST; item < n_round; item += stride) {
        const bool live = item < n;
        const size_t q = live ? SAMPLE_ROW(item) : 0;
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
