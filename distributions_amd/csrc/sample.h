// Group::sample_value (dd.hpp:188-199, bb.hpp:154-160, gp.hpp:166-172,
// nich.hpp:204-210, bnb.hpp:168-174, dpd.hpp:275-305): one draw from a
// group's posterior predictive, the law whose log density score_value
// returns (for BNB that score plus the binomial coefficient it leaves out).
// Inline host/device code in the manner of models.h: the host entry
// dist_group_sample_value and the kernels of kernels_sample.h call the very
// same function.
//
// All arithmetic is binary64 over the statistics promoted from their words,
// with the platform's log, exp, sqrt and lgamma (NOT special.h's fast
// functions, which are approximations pinned to the reference's scorers).
// The random numbers are counter-based: cell (row, f) of seed_state owns the
// stream  mix64(key + j), j = 0, 1, ...  with
//   key = mix64(mix64(mix64(seed_state) ^ row) ^ (f + 1)),
// so a rejection loop may take as many as it needs and no two cells share
// any.  Every loop is bounded; a cell whose loop ran out says so.
#pragma once

#include <math.h>

#include "models.h"

namespace dist {

// what the cell draw needs of a Shared
struct SampleShared {
    int kind;
    int dim;
    float p[4];
    const float * w;   // DD: alphas[dim]; DPD: betas[dim]
};

// the hyper-parameter arrays are wave-uniform on the device: scalar loads
#if defined(__HIP_DEVICE_COMPILE__)
#define DIST_SAMPLE_W(p, v)                                                  \
    (((const float __attribute__((address_space(4))) *)(unsigned long long)(p))[v])
#else
#define DIST_SAMPLE_W(p, v) ((p)[v])
#endif

DIST_HD uint64_t sample_mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct SampleStream {
    uint64_t key;
    uint64_t j;
    bool exhausted;   // a bounded loop ran out of tries
};

DIST_HD SampleStream sample_stream(uint32_t seed_state, uint64_t row, int f) {
    SampleStream s;
    s.key = sample_mix64(sample_mix64(sample_mix64((uint64_t)seed_state) ^ row)
                         ^ (uint64_t)(f + 1));
    s.j = 0;
    s.exhausted = false;
    return s;
}

// in (0, 1)
DIST_HD double sample_u(SampleStream & s) {
    const uint64_t w = sample_mix64(s.key + s.j);
    s.j += 1;
    return ((double)(w >> 11) + 0.5) * 0x1p-53;
}

// Marsaglia's polar method
DIST_HD double sample_normal(SampleStream & s) {
    for (int tries = 0; tries < 64; ++tries) {
        const double a = 2.0 * sample_u(s) - 1.0;
        const double b = 2.0 * sample_u(s) - 1.0;
        const double r = a * a + b * b;
        if (r > 0.0 && r < 1.0) return a * sqrt(-2.0 * log(r) / r);
    }
    s.exhausted = true;
    return 0.0;
}

// Marsaglia-Tsang, scale 1
DIST_HD double sample_gamma(SampleStream & s, double a) {
    double boost = 1.0;
    if (a < 1.0) {
        boost = exp(log(sample_u(s)) / a);
        a += 1.0;
    }
    const double d = a - 1.0 / 3.0;
    const double c = 1.0 / sqrt(9.0 * d);
    for (int tries = 0; tries < 64; ++tries) {
        const double z = sample_normal(s);
        double v = 1.0 + c * z;
        if (v <= 0.0) continue;
        v = v * v * v;
        const double w = sample_u(s);
        const double z2 = z * z;
        if (w < 1.0 - 0.0331 * (z2 * z2)) return d * v * boost;
        if (log(w) < 0.5 * z2 + d * (1.0 - v + log(v))) return d * v * boost;
    }
    s.exhausted = true;
    return d * boost;
}

// counts saturate at 2^31 - 1
DIST_HD uint32_t sample_count_word(double k) {
    if (!(k < 2147483647.0)) return 2147483647u;
    return k < 0.0 ? 0u : (uint32_t)k;
}

// inversion below 10, Hoermann's PTRS from there
DIST_HD uint32_t sample_poisson(SampleStream & s, double lam) {
    if (!(lam < 2147483648.0)) return 2147483647u;
    if (lam < 10.0) {
        double p = exp(-lam);
        const double w = sample_u(s);
        int k = 0;
        double cum = p;
        while (w > cum && k < 1000) {
            k += 1;
            p *= lam / (double)k;
            cum += p;
        }
        return (uint32_t)k;
    }
    const double b = 0.931 + 2.53 * sqrt(lam);
    const double a = -0.059 + 0.02483 * b;
    const double ia = 1.1239 + 1.1328 / (b - 3.4);
    const double vr = 0.9277 - 3.6224 / (b - 2.0);
    const double log_lam = log(lam);
    for (int tries = 0; tries < 64; ++tries) {
        const double U = sample_u(s) - 0.5;
        const double V = sample_u(s);
        const double us = 0.5 - fabs(U);
        const double k = floor((2.0 * a / us + b) * U + lam + 0.43);
        if (us >= 0.07 && V <= vr) return sample_count_word(k);
        if (k < 0.0 || (us < 0.013 && V > us)) continue;
        if (log(V) + log(ia) - log(a / (us * us) + b)
            <= -lam + k * log_lam - lgamma(k + 1.0))
            return sample_count_word(k);
    }
    s.exhausted = true;
    return sample_count_word(floor(lam));
}

// One cell: a draw of feature f's value for `row` from the predictive of the
// group with statistics `st` (and, for the categorical kinds, the counts
// cnt[0..dim)).  *exhausted is set when a bounded loop ran out (and left
// alone otherwise).
DIST_HD uint32_t sample_cell_word(int kind, const SampleShared & sh,
                                  const Stats & st, const int32_t * cnt,
                                  uint32_t seed_state, uint64_t row, int f,
                                  bool * exhausted) {
    SampleStream s = sample_stream(seed_state, row, f);
    uint32_t word = 0u;
    switch (kind) {
    case DIST_DD: {
        double total = 0.0;
        for (int v = 0; v < sh.dim; ++v)
            total += (double)DIST_SAMPLE_W(sh.w, v) + (double)cnt[v];
        double t = sample_u(s) * total;
        word = (uint32_t)(sh.dim - 1);
        for (int v = 0; v < sh.dim; ++v) {
            t -= (double)DIST_SAMPLE_W(sh.w, v) + (double)cnt[v];
            if (t < 0.0) {
                word = (uint32_t)v;
                break;
            }
        }
        break;
    }
    case DIST_DPD: {
        const double alpha = (double)sh.p[0];
        const double other = (double)sh.p[1] * alpha;
        double total = 0.0;
        for (int v = 0; v < sh.dim; ++v)
            total += (double)DIST_SAMPLE_W(sh.w, v) * alpha + (double)cnt[v];
        if (other > 0.0) total += other;
        double t = sample_u(s) * total;
        word = other > 0.0 ? DIST_DPD_OTHER : (uint32_t)(sh.dim - 1);
        for (int v = 0; v < sh.dim; ++v) {
            t -= (double)DIST_SAMPLE_W(sh.w, v) * alpha + (double)cnt[v];
            if (t < 0.0) {
                word = (uint32_t)v;
                break;
            }
        }
        break;
    }
    case DIST_BB: {
        const double a = (double)sh.p[0] + (double)st.i0;
        const double b = (double)sh.p[1] + (double)st.i1;
        const double p = a / (a + b);
        word = sample_u(s) < p ? 1u : 0u;
        break;
    }
    case DIST_GP: {
        const double shape = (double)sh.p[0] + (double)st.i1;
        const double rate = (double)sh.p[1] + (double)st.i0;
        word = sample_poisson(s, sample_gamma(s, shape) / rate);
        break;
    }
    case DIST_BNB: {
        const double r = (double)sh.p[2];
        const double a = (double)sh.p[0] + r * (double)st.i0;
        const double b = (double)sh.p[1] + (double)st.i1;
        const double x = sample_gamma(s, a);
        const double y = sample_gamma(s, b);
        double p = x / (x + y);
        if (x == 0.0 && y == 0.0) p = sample_u(s) < a / (a + b) ? 1.0 : 0.0;
        word = sample_poisson(s, sample_gamma(s, r) * (1.0 - p) / p);
        break;
    }
    default: {   // DIST_NICH
        const double mu = (double)sh.p[0], kappa = (double)sh.p[1];
        const double sigmasq = (double)sh.p[2], nu = (double)sh.p[3];
        const double n = (double)st.i0, mean = (double)st.f0;
        const double ctv = (double)st.f1;
        const double kn = kappa + n;
        const double mun = (kappa * mu + mean * n) / kn;
        const double nun = nu + n;
        const double dm = mu - mean;
        const double sn =
            (nu * sigmasq + ctv + n * kappa * (dm * dm) / kn) / nun;
        const double z = sample_normal(s);
        const double g = sample_gamma(s, nun / 2.0);
        const float x = (float)(mun + sqrt(sn * (kn + 1.0) / kn) * z
                                          * sqrt(nun / (2.0 * g)));
        word = f2u(x);
        break;
    }
    }
    if (s.exhausted) *exhausted = true;
    return word;
}

}  // namespace dist
