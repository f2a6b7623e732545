// The certificate of the value-sorted sampler's prefix-sum search
// (k_vs_search, kernels_vs.h).  Plain C++: the device build includes it, and
// so does a host program (tests/test_certified_search_cpu.py holds it to a
// float32 chain written in numpy).
//
// What is certified.  k_vs_sample answers one question per row with a chain
// of float subtractions (vs_sum_and_scan):
//     t_{-1} = t0 = fl(tot * u),   t_k = fl(t_{k-1} - e_k),  k = 0 .. K-1,
//     answer = min(first k with t_k <= 0, K - 1),
// where e_k >= 0 is the value's likelihood vector L[x][k] with the row's own
// slot g replaced by l_own.  The search answers it from a float64 prefix sum
// shared by all rows of the value,
//     S_k = C[k] + [k >= g] (l_own - L[x][g]),    r_k = t0 - S_k,
// and the certificate decides whether the chain is PROVEN to give the same
// index.  A row it does not certify runs the chain.
//
// Float mode.  The library is built with -fgpu-flush-denormals-to-zero and
// -ffp-contract=off: a float32 subtraction rounds to nearest even, treats a
// denormal input as zero and returns zero for a denormal result; no FMA is
// formed.  Float64 keeps its denormals.  The proof holds for that mode and
// for plain IEEE float32 alike (the host test runs both).
//
// Proof.  Let m be the chain's first index with t_m <= 0 (none: m = K), and
// err_k = |t_k - r_k| in real numbers, r_k with the exact prefix sum.
//  (1) Monotone.  e_k >= 0, rounding is monotone and flushing moves a value
//      towards zero, so t_k never increases and neither does r_k: t_j > 0
//      for every j < m, t_j <= 0 for every j >= m.
//  (2) One step below the crossing, k < m.  The result is a positive normal
//      float, so its rounding error is at most half an ulp of the result:
//      <= 2^-24 t_k.  A denormal e_k read as zero adds less than 2^-126.
//  (3) The crossing step, k = m.  The exact difference lies in [-e_m, 0] up
//      to the error carried so far (t_{m-1} > 0 goes in), so |t_m| <=
//      e_m (1 + 2^-24) and the step rounds by <= 2^-24 max(t0, e_m); here
//      <= 2^-24 emax (1 + 2^-24), emax >= every e_k.  A denormal result
//      flushed to zero moves by less than 2^-126, and zero is "crossed".
//  (4) The sum.  For k <= m, with a = 2^-125 per step for (2) and (3):
//        err_k <= 2^-24 (sum_{i<=k, i<m} t_i + [k = m] emax') + (k+1) a,
//        t_i <= r_i + err_i.
//      Where r_i > 0 for all i < k (the decision below establishes it),
//      r_k > -emax, and sum_{i<=k} r_i = (k+1) t0 - D_k =: R_k with D_k the
//      prefix sum of the S_i; the partial sums R_i, i <= k, are at most
//      R_k + emax.  With G = max_{i<=k} err_i this gives
//        G (1 - (k+1) 2^-24) <= 2^-24 (R_k + 2 emax) + (k+1) a,
//      and k + 1 <= 2^13 (the tables hold at most 8192 groups) turns the
//      factor into 1 + 2^-10 with room for (3)'s 2^-24 and for D_k's own
//      rounding (float64 sums of at most 2^13 terms: relative 2^-40 of
//      D_k <= 2^26 emax, against R_k + 2 emax >= 2 emax).
//  (5) The float64 prefix.  C[k] is a sum of k+1 non-negative floats in
//      float64, in any order: off by <= (k+1) 2^-53 C[k]; the two or three
//      float64 operations that form r_k from it add <= 3 * 2^-53 (t0 + S_k).
//      Both are inside (k+1) 2^-51 (t0 + S_k).
//  (6) The absolute term (k+1) 2^-120 is (4)'s (k+1) a with room to spare.
//  So E_k below bounds err_k for every k <= m that the decision asks about,
//  and E_j <= E_k for j <= k while the r_i are positive (R_j grows with j).
//  Decision, for the search's k (first k <= K-2 with r_k <= 0, else K-1):
//   - r_{k-1} > E_{k-1} (asked when k > 0) proves m >= k: if m <= k-1 then
//     t_m >= r_m - E_m >= r_{k-1} - E_{k-1} > 0, against t_m <= 0.
//   - r_k < -E_k (asked when k <= K-2) proves m <= k: if m > k then t_k > 0
//     and t_k <= r_k + E_k < 0.
//   - k = K-1 needs the first alone: the chain's index is clamped to K-1.
//   - t0 <= 0 (u = 0, or a product flushed to zero) gives t_0 <= 0 whatever
//     e_0 is: index 0, no rounding involved.  K = 1 has one answer.
//  The search itself needs no proof: whichever k it proposes, the two
//  inequalities hold only for the chain's own index.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define VS_CERTIFY_HD __host__ __device__
#else
#define VS_CERTIFY_HD
#endif

namespace dist {

// The largest group count the bound is proven for ((4): k + 1 <= 2^13).
constexpr int kVsCertifyMaxK = 8192;

// E_k: how far the float chain's t_k can be from r_k = t0 - S_k as float64
// computes it.  t0 = fl(tot * u); S_k and D_k are the row's prefix sum and
// prefix sum of prefix sums at k, own-slot correction included; emax >= 1 and
// >= every entry and own-slot value; slack scales the bound by 2^slack (tests
// only: small shapes reach the uncertified path).
VS_CERTIFY_HD inline double vs_certify_bound(float t0, int k, double S_k,
                                             double D_k, double emax,
                                             int slack) {
    const double n = (double)(k + 1);
    double R = n * (double)t0 - D_k;
    if (!(R > 0.0)) R = 0.0;
    const double chain = 0x1p-24 * (R + 2.0 * emax) * (1.0 + 0x1p-10);
    const double prefix = n * 0x1p-51 * ((double)t0 + S_k);
    const double flushed = n * 0x1p-120;
    return ldexp(chain + prefix + flushed, slack);
}

// The search, one step: [lo, hi] keeps the first k <= K-2 with r_k <= 0 (or
// K-1).  C[k]: float64 inclusive prefix sums of the value's vector; g,
// delta = l_own - L[x][g]: the row's own slot and what it changes; t = t0.
// Branch-free, so that a thread's rows take their steps side by side.
VS_CERTIFY_HD inline void vs_search_step(const double * C, int g,
                                         double delta, double t, int & lo,
                                         int & hi) {
    const int mid = (lo + hi) >> 1;   // (< K - 1 while lo < hi)
    const double S = C[mid] + (mid >= g ? delta : 0.0);
    const bool open = lo < hi, up = S >= t;
    hi = open && up ? mid : hi;
    lo = open && !up ? mid + 1 : lo;
}
// where the search starts: the whole range, or index 0 where that is the
// answer without a search (one group; t0 <= 0)
VS_CERTIFY_HD inline int vs_search_top(int K, float t0) {
    return K <= 1 || !(t0 > 0.f) ? 0 : K - 1;
}
// The decision for the index k the search ended at: does the chain provably
// give it?  D[k]: float64 inclusive prefix sums of C.
VS_CERTIFY_HD inline bool vs_certify_decide(const double * C,
                                            const double * D, int K, int g,
                                            double delta, float t0,
                                            double emax, int slack, int k) {
    if (vs_search_top(K, t0) == 0) return k == 0;
    const double t = (double)t0;
    const int j = k > 0 ? k - 1 : 0;
    const double Sk = C[k] + (k >= g ? delta : 0.0);
    const double Dk = D[k] + (k >= g ? (double)(k - g + 1) * delta : 0.0);
    const double Sj = C[j] + (j >= g ? delta : 0.0);
    const double Dj = D[j] + (j >= g ? (double)(j - g + 1) * delta : 0.0);
    const bool below =
        (t - Sk) < -vs_certify_bound(t0, k, Sk, Dk, emax, slack);
    const bool above =
        (t - Sj) > vs_certify_bound(t0, j, Sj, Dj, emax, slack);
    return delta == delta && emax >= 1.0 && k >= 0 && k < K
           && (k >= K - 1 || below) && (k == 0 || above);
}
// Search and decide; steps: any count with 2^steps >= K.  Returns the index
// and sets *certified when the chain provably gives it.
VS_CERTIFY_HD inline int vs_certified_search(const double * C,
                                             const double * D, int K, int g,
                                             double delta, float t0,
                                             double emax, int slack,
                                             int steps, bool * certified) {
    int lo = 0, hi = vs_search_top(K, t0);
    for (int s = 0; s < steps; ++s)
        vs_search_step(C, g, delta, (double)t0, lo, hi);
    *certified = lo == hi
                 && vs_certify_decide(C, D, K, g, delta, t0, emax, slack, lo);
    return lo;
}

}   // namespace dist
