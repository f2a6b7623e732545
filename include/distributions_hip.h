/* distributions_hip.h -- C ABI of libdistributions_hip.so
 *
 * MI355X (gfx950) implementation of the collapsed-Gibbs mixture hot path of
 * forcedotcom/distributions v2.0.28.  The reference has no C ABI: its boundary
 * is C++ templates (include/distributions/{mixture,clustering}.hpp,
 * the models headers) wrapped by Cython (distributions/lp/).  Each entry point below
 * names the reference member it stands in for (paths relative to the
 * reference root).  include/distributions_hip.hpp re-presents these as the
 * reference's C++ classes; distributions_amd/lp re-presents them as the
 * reference's Python classes.
 *
 * Conventions
 *   - every call returns 0 on success, non-zero on error; dist_last_error()
 *     then holds the message (the reference throws std::runtime_error under
 *     DIST_THROW_ON_ERROR, common.hpp:49-57).  Bounds are always checked.
 *   - numeric state (sufficient statistics, score caches) lives in HBM; host
 *     pointers are caller-owned and copied in/out, like the numpy<->VectorFloat
 *     copies of lp/vector.pyx:33-47.  Pointers named *_dev are device memory.
 *   - values cross the ABI as 32-bit words: int for DirichletDiscrete /
 *     BetaBernoulli / GammaPoisson / DirichletProcessDiscrete, IEEE float bits
 *     for NormalInverseChiSq.
 *   - group ids are "packed" ids (mixture.hpp:41-46) unless named global.
 */
#ifndef DISTRIBUTIONS_HIP_H
#define DISTRIBUTIONS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIST_ABI_VERSION 1

enum dist_kind {
    DIST_DD = 0,   /* models/dd.hpp   DirichletDiscrete<256>          */
    DIST_BB = 1,   /* models/bb.hpp   BetaBernoulli                   */
    DIST_GP = 2,   /* models/gp.hpp   GammaPoisson                    */
    DIST_NICH = 3, /* models/nich.hpp NormalInverseChiSq              */
    DIST_DPD = 4,  /* models/dpd.hpp  DirichletProcessDiscrete (dense
                      value remap: value v in [0,dim), OTHER = 2^32-1) */
    DIST_BNB = 5   /* models/bnb.hpp  BetaNegativeBinomial            */
};

#define DIST_DD_MAX_DIM 256
#define DIST_DPD_OTHER 0xFFFFFFFFu
#define DIST_MAX_FEATURES 8

/* Model::Shared (dd.hpp:57-86, bb.hpp:54-76, gp.hpp:52-81, nich.hpp:52-95,
 * dpd.hpp:59-153) */
typedef struct dist_shared {
    int kind;
    int dim;             /* DD: dim; DPD: number of known values            */
    float p[4];          /* BB: alpha,beta | GP: alpha,inv_beta |
                            NICH: mu,kappa,sigmasq,nu | DPD: alpha,beta0 |
                            BNB: alpha,beta,r (r a positive integer)        */
    float alphas[DIST_DD_MAX_DIM]; /* DD                                    */
    const float * betas; /* DPD: betas[dim], host pointer, copied           */
} dist_shared_t;

/* Model::Group as 32-bit words (dd.hpp:89-93, bb.hpp:79-82, gp.hpp:84-88,
 * nich.hpp:98-102, dpd.hpp:157-158):
 *   DD / DPD: { count_sum, counts[dim] }     BB:   { heads, tails }
 *   GP:       { count, sum, log_prod(f32) }  NICH: { count, mean(f32),
 *                                                    count_times_variance(f32) }
 *   BNB:      { count, sum }                                  (bnb.hpp:87-89) */
size_t dist_group_words(const dist_shared_t * shared);

int dist_abi_version(void);
const char * dist_last_error(void);
int dist_device_count(int * count);
int dist_set_device(int device);
int dist_synchronize(void);
/* The HIP stream (hipStream_t, NULL = the default stream) that carries every
 * launch and copy the CALLING THREAD makes from now on.  Independent engines
 * driven from different host threads on different streams overlap on the
 * device; objects must be used on the stream they were created on (or after
 * the caller has synchronised the two). */
int dist_set_stream(void * hip_stream);

/* ---- entropy: rng_t = std::default_random_engine (random_fwd.hpp:34) ----
 * The engine state is one word; sample_unif01 (random.hpp:47-50) consumes
 * exactly one step. */
uint32_t dist_rng_seed(uint64_t seed);            /* engine.seed(seed)      */
uint32_t dist_rng_next(uint32_t * state);         /* engine()               */
float dist_rng_unif01(uint32_t * state);          /* sample_unif01          */
uint32_t dist_rng_jump(uint32_t state, uint64_t steps);

/* ---- special.hpp / vector_math.hpp on device (host arrays in/out) -------- */
int dist_vector_log(size_t n, const float * in, float * out);      /* vector_math.cc:224-255 */
int dist_vector_exp(size_t n, const float * in, float * out);      /* :190-221 */
int dist_vector_lgamma(size_t n, const float * in, float * out);   /* :257-272 */
int dist_vector_lgamma_nu(size_t n, const float * in, float * out);/* :275-291 */
int dist_vector_log_factorial(size_t n, const uint32_t * in, float * out); /* special.hpp:208-214 */

/* ---- discrete sampling (random.hpp:316-392, random.cc:77-128) ------------ */
/* sample_from_scores_overwrite: scores[n] (host) become likelihoods */
int dist_sample_from_scores_overwrite(uint32_t * rng_state, size_t n,
                                      float * scores, size_t * sample_out);
int dist_scores_to_likelihoods(size_t n, float * scores, float * total_out);
int dist_sample_from_likelihoods(uint32_t * rng_state, size_t n,
                                 const float * likelihoods, float total,
                                 size_t * sample_out);
int dist_log_sum_exp(size_t n, const float * scores, float * out);

/* ---- Clustering<int>::PitmanYor (clustering.hpp:58-123) ------------------ */
int dist_py_score_add_value(float alpha, float d, int group_size,
                            int nonempty_group_count, int sample_size,
                            int empty_group_count, float * out);
int dist_py_score_remove_value(float alpha, float d, int group_size,
                               int nonempty_group_count, int sample_size,
                               int empty_group_count, float * out);

/* sample_assignments(size, rng): sequential CRP/Pitman-Yor draw of `size`
 * group ids (clustering.cc:67-142); host-side like the reference */
int dist_py_sample_assignments(float alpha, float d, int size,
                               uint32_t * rng_state, int * assignments_out);
/* score_counts(counts): log probability of a partition (clustering.cc:152-183) */
int dist_py_score_counts(float alpha, float d, const int * counts,
                         size_t group_count, float * out);

/* ---- Clustering<int>::LowEntropy (clustering.hpp:245-331) ----------------
 * dataset_size is the model; nonempty_group_count is accepted and unused, as
 * in the reference.  score_counts: clustering.cc:229-248 (n log n terms summed
 * in binary64, 1e-6 relative); log_partition_function: clustering.cc:204-215.
 * sample_assignments: clustering.cc:250-283, host-side like the reference
 * (its totals follow the release build's vector_sum association). */
int dist_le_score_add_value(int dataset_size, int group_size,
                            int nonempty_group_count, int sample_size,
                            int empty_group_count, float * out);
int dist_le_score_remove_value(int dataset_size, int group_size,
                               int nonempty_group_count, int sample_size,
                               int empty_group_count, float * out);
int dist_le_log_partition_function(int sample_size, float * out);
int dist_le_sample_assignments(int dataset_size, int sample_size,
                               uint32_t * rng_state, int * assignments_out);
int dist_le_score_counts(int dataset_size, const int * counts,
                         size_t group_count, float * out);
/* LowEntropy::Mixture = MixtureDriver<LowEntropy, int> (mixture.hpp:48-163) */
typedef struct dist_le_mixture dist_le_mixture_t;
dist_le_mixture_t * dist_le_mixture_create(void);
void dist_le_mixture_destroy(dist_le_mixture_t * m);
int dist_le_mixture_init(dist_le_mixture_t * m, const int * counts,
                         size_t group_count);                 /* mixture.hpp:59-71   */
int dist_le_mixture_add_value(dist_le_mixture_t * m, size_t groupid,
                              int * added_out);               /* mixture.hpp:73-92   */
int dist_le_mixture_remove_value(dist_le_mixture_t * m, size_t groupid,
                                 int * removed_out);          /* mixture.hpp:94-122  */
int dist_le_mixture_score_value(const dist_le_mixture_t * m, int dataset_size,
                                float * scores, size_t size); /* mixture.hpp:124-141 */
int dist_le_mixture_score_data(const dist_le_mixture_t * m, int dataset_size,
                               float * out);                  /* mixture.hpp:143-145 */
size_t dist_le_mixture_size(const dist_le_mixture_t * m);
size_t dist_le_mixture_sample_size(const dist_le_mixture_t * m);
int dist_le_mixture_counts(const dist_le_mixture_t * m, int * out);

/* ---- PitmanYor::Mixture = CachedMixture (clustering.hpp:126-234) --------- */
typedef struct dist_py_mixture dist_py_mixture_t;
dist_py_mixture_t * dist_py_mixture_create(void);
void dist_py_mixture_destroy(dist_py_mixture_t * m);
/* counts() = counts; init(model)                       clustering.hpp:151-161 */
int dist_py_mixture_init(dist_py_mixture_t * m, float alpha, float d,
                         const int * counts, size_t group_count);
/* add_value(model, groupid) -> group was empty         clustering.hpp:163-176 */
int dist_py_mixture_add_value(dist_py_mixture_t * m, float alpha, float d,
                              size_t groupid, int * added_out);
/* remove_value(model, groupid) -> group became empty   clustering.hpp:178-193 */
int dist_py_mixture_remove_value(dist_py_mixture_t * m, float alpha, float d,
                                 size_t groupid, int * removed_out);
/* score_value(model, scores): OVERWRITES scores[size]  clustering.hpp:195-208 */
int dist_py_mixture_score_value(const dist_py_mixture_t * m, float alpha,
                                float d, float * scores, size_t size);
/* score_data(model) = model.score_counts(counts())      clustering.hpp:210-212 */
int dist_py_mixture_score_data(const dist_py_mixture_t * m, float alpha,
                               float d, float * out);
size_t dist_py_mixture_size(const dist_py_mixture_t * m);           /* counts().size() */
size_t dist_py_mixture_sample_size(const dist_py_mixture_t * m);    /* sample_size()   */
int dist_py_mixture_counts(const dist_py_mixture_t * m, int * out); /* counts()        */
/* empty_groupids(): writes at most cap ids, returns how many exist */
size_t dist_py_mixture_empty_groupids(const dist_py_mixture_t * m,
                                      size_t * out, size_t cap);

/* ---- Model::Mixture = MixtureSlave<Model, ...> (mixture.hpp:340-450) ----- */
typedef struct dist_mixture dist_mixture_t;
dist_mixture_t * dist_mixture_create(const dist_shared_t * shared);
void dist_mixture_destroy(dist_mixture_t * m);
int dist_mixture_clear(dist_mixture_t * m);                        /* groups().clear()      */
int dist_mixture_append(dist_mixture_t * m, const uint32_t * group);/* groups().push_back(g) */
int dist_mixture_get_group(const dist_mixture_t * m, size_t groupid,
                           uint32_t * group_out);                  /* groups(i) (copy)      */
size_t dist_mixture_size(const dist_mixture_t * m);                /* groups().size()       */
int dist_mixture_init(dist_mixture_t * m);                         /* init        :354-359  */
int dist_mixture_add_group(dist_mixture_t * m);                    /* add_group   :361-368  */
int dist_mixture_remove_group(dist_mixture_t * m, size_t groupid); /* remove_group:370-375  */
int dist_mixture_add_value(dist_mixture_t * m, size_t groupid,
                           uint32_t value);                        /* add_value   :377-384  */
int dist_mixture_remove_value(dist_mixture_t * m, size_t groupid,
                              uint32_t value);                     /* remove_value:386-398  */
int dist_mixture_score_value_group(const dist_mixture_t * m, size_t groupid,
                                   uint32_t value, float * out);   /* :400-414 */
/* score_value: ACCUMULATES into scores_accum[size]                   :416-425 */
int dist_mixture_score_value(const dist_mixture_t * m, uint32_t value,
                             float * scores_accum, size_t size);

/* score_data: log marginal likelihood of all groups' data    mixture.hpp:427-431
 * Accumulated in the reference's own float order (per-value chains closed by
 * vector_sum for DirichletDiscrete, one chain over the groups otherwise):
 * bit-exact against a float restatement of its loops.  DirichletProcessDiscrete
 * walks a hash map in the reference: its terms are summed in binary64,
 * 1e-5 relative. */
int dist_mixture_score_data(const dist_mixture_t * m, float * out);
/* score_data_grid: scores_out[i] = score_data under candidate shareds[i]
 * (hyper-parameter grid, mixture.hpp:433-438 / 238-247; DirichletDiscrete
 * carries alpha_sum from candidate to candidate like dd.hpp:259-284,320-344).
 * Every candidate is scored in the same launches; same contract. */
int dist_mixture_score_data_grid(const dist_mixture_t * m,
                                 const dist_shared_t * shareds, size_t n,
                                 float * scores_out);

/* score_value for n values in ONE launch (extension; mixture.hpp:416-425 per
 * value): scores_accum[r * ld + k] accumulates the score of values[r] in group
 * k, bit for bit what n calls of dist_mixture_score_value leave.  The per-value
 * call costs a launch and a round trip (measured with the reference's own
 * harness: 0.03 cells/us at every K); this is the member to
 * use between one value and a whole dist_gibbs_t. */
int dist_mixture_score_values(const dist_mixture_t * m,
                              const uint32_t * values, size_t n,
                              float * scores_accum, size_t ld);
/* Mixture::validate (mixture.hpp:440-444; dd.hpp:447-455 and the other value
 * scorers'): group counts agree, count_sum == sum of counts, and the value
 * scorer's cache equals Scorer::init of the statistics bit for bit
 * (recomputed on the device).  Non-zero + dist_last_error() otherwise. */
int dist_mixture_validate(const dist_mixture_t * m);

/* ---- Model::Group scalar API (host side, O(1); dd.hpp:113-199 etc.) ------ */
int dist_group_init(const dist_shared_t * shared, uint32_t * group);
int dist_group_add_value(const dist_shared_t * shared, uint32_t * group,
                         uint32_t value);
int dist_group_remove_value(const dist_shared_t * shared, uint32_t * group,
                            uint32_t value);
int dist_group_score_value(const dist_shared_t * shared,
                           const uint32_t * group, uint32_t value,
                           float * out);
int dist_group_score_data(const dist_shared_t * shared, const uint32_t * group,
                          float * out);
/* Group::sample_value (dd.hpp:188-199, bb.hpp:154-160, gp.hpp:166-172,
 * nich.hpp:204-210, bnb.hpp:168-174, dpd.hpp:275-305): n draws from the
 * group's posterior predictive -- the law whose log density
 * dist_group_score_value returns; for BetaNegativeBinomial that score plus
 * log C(x + r - 1, x), which the reference's score leaves out and a sampler
 * cannot.  words_out[i] is the draw of cell (row_first + i, feature): the
 * counter-based stream keyed by (seed_state, row, feature) and the binary64
 * arithmetic of csrc/sample.h, the very inline function the kernels of
 * dist_gibbs_sample_rows call.  Counts, or float bits for NormalInverseChiSq;
 * DIST_DPD_OTHER where a DirichletProcessDiscrete draw leaves the table.  Host
 * only, needs no device.  Fails when a bounded rejection loop runs out of
 * tries (NaN hyper-parameters). */
int dist_group_sample_value(const dist_shared_t * shared,
                            const uint32_t * group, uint32_t seed_state,
                            uint64_t row_first, size_t n, int feature,
                            uint32_t * words_out);
/* Model::Scorer (dd.hpp:222-245, bb.hpp:185-205, gp.hpp:198-217,
 * nich.hpp:239-259, bnb.hpp:195-223, dpd.hpp:309-341): init caches what eval
 * needs of ONE group's statistics, eval scores a value from the cache -- the
 * per-group ("naive") counterpart of the Mixture's vectorised score_value,
 * the other half of benchmarks/mixture.cc:41-74,119-135.  Host side, O(dim)
 * / O(1); the state is dist_scorer_words(shared) floats owned by the caller:
 * alpha_sum and alphas[dim] for DirichletDiscrete, the logarithm for OTHER
 * and for each of the dim values for DirichletProcessDiscrete, the scalar
 * members of the reference's Scorer otherwise. */
size_t dist_scorer_words(const dist_shared_t * shared);
int dist_scorer_init(const dist_shared_t * shared, const uint32_t * group,
                     float * state);
int dist_scorer_eval(const dist_shared_t * shared, const float * state,
                     uint32_t value, float * out);

/* ---- DirichletProcessDiscrete::Shared, the stick-breaking side -------------
 * (dpd.hpp:59-101; lp/models/_dpd.pyx:31-45).  Host side like the reference's:
 * gamma, alpha, beta0, the betas of the values that exist and how many rows
 * carry each.  A value owns a DENSE SLOT for life (the index groups and the
 * kernels count it under); a value whose last row leaves gives its beta back
 * to beta0 and its slot to the next new value.
 *   add_value     dpd.hpp:66-74  a first row of a new value breaks
 *                 beta0 * sample_beta_safe(rng, 1, gamma, MIN_BETA) off the stick
 *   remove_value  dpd.hpp:76-83
 *   realize       dpd.hpp:85-101 new values until beta0 <= 1e-4 or 9 999 exist,
 *                 the rest of the stick to one last value; beta0 = 0
 *   load          protobuf_load dpd.hpp:103-124 (beta0 = max(0, 1 - sum betas))
 *   view          the dist_shared_t the mixtures take: dim = slots, betas by
 *                 slot (0 for a free slot); the pointer is the object's own
 *                 storage, valid until its next mutation (`version` moves)
 *   slot          value -> dense slot (OTHER -> OTHER); unknown values fail
 *   dump          by slot: value (0xFFFFFFFF = free), beta, count
 * Entropy: rng_t's one word of state, advanced as libstdc++'s
 * std::gamma_distribution<double> over std::default_random_engine advances it
 * (random.hpp:87-119). */
typedef struct dist_dpd_shared dist_dpd_shared_t;
dist_dpd_shared_t * dist_dpd_shared_create(void);
void dist_dpd_shared_destroy(dist_dpd_shared_t * s);
int dist_dpd_shared_copy(dist_dpd_shared_t * dst,
                         const dist_dpd_shared_t * src);  /* Shared's copy  */
int dist_dpd_shared_load(dist_dpd_shared_t * s, float gamma, float alpha,
                         const uint32_t * values, const float * betas,
                         const int * counts, size_t n);
int dist_dpd_shared_add_value(dist_dpd_shared_t * s, uint32_t value,
                              uint32_t * rng_state);
int dist_dpd_shared_remove_value(dist_dpd_shared_t * s, uint32_t value);
int dist_dpd_shared_realize(dist_dpd_shared_t * s, uint32_t * rng_state);
size_t dist_dpd_shared_slots(const dist_dpd_shared_t * s);
size_t dist_dpd_shared_size(const dist_dpd_shared_t * s);
uint64_t dist_dpd_shared_version(const dist_dpd_shared_t * s);
int dist_dpd_shared_params(const dist_dpd_shared_t * s, float * gamma,
                           float * alpha, float * beta0);
int dist_dpd_shared_view(const dist_dpd_shared_t * s, dist_shared_t * out);
int dist_dpd_shared_slot(const dist_dpd_shared_t * s, uint32_t value,
                         uint32_t * slot_out);
int dist_dpd_shared_dump(const dist_dpd_shared_t * s, uint32_t * values,
                         float * betas, int * counts);
/* sample_gamma / sample_beta_safe (random.hpp:87-97,110-119) over rng_t */
int dist_sample_gamma(uint32_t * rng_state, float alpha, float beta,
                      float * out);
int dist_sample_beta_safe(uint32_t * rng_state, float alpha, float beta,
                          float min_value, float * out);

/* ---- protobuf wire format of Shared / Group -------------------------------
 * The messages of distributions/io/schema.proto (package
 * protobuf.distributions) as bytes, what Group::protobuf_dump / protobuf_load
 * exchange through generated classes in the reference (dd.hpp:94-111,
 * bb.hpp:84-93, gp.hpp:90-101, nich.hpp:104-115, dpd.hpp:161-180) -- here
 * without libprotobuf.  dump: buf == NULL asks for the size (*len_out).
 * keys (DirichletProcessDiscrete only): keys[i] = the value that dense index
 * i stands for; NULL = identity. */
int dist_group_protobuf_dump(const dist_shared_t * shared,
                             const uint32_t * group, const uint32_t * keys,
                             uint8_t * buf, size_t cap, size_t * len_out);
int dist_group_protobuf_load(const dist_shared_t * shared,
                             const uint32_t * keys, const uint8_t * data,
                             size_t len, uint32_t * group_out);
/* Shared messages of DD / BB / GP / NICH (DPD's Shared carries the
 * stick-breaking state, which lives in the lp layer) */
int dist_shared_protobuf_dump(const dist_shared_t * shared, uint8_t * buf,
                              size_t cap, size_t * len_out);
int dist_shared_protobuf_load(int kind, const uint8_t * data, size_t len,
                              dist_shared_t * shared_out);

/* ---- MixtureIdTracker (mixture.hpp:460-521) ------------------------------ */
typedef struct dist_id_tracker dist_id_tracker_t;
dist_id_tracker_t * dist_id_tracker_create(void);
void dist_id_tracker_destroy(dist_id_tracker_t * t);
int dist_id_tracker_init(dist_id_tracker_t * t, size_t group_count);
int dist_id_tracker_add_group(dist_id_tracker_t * t);
int dist_id_tracker_remove_group(dist_id_tracker_t * t, uint32_t packed);
int dist_id_tracker_packed_to_global(const dist_id_tracker_t * t,
                                     uint32_t packed, uint32_t * global_out);
int dist_id_tracker_global_to_packed(const dist_id_tracker_t * t,
                                     uint32_t global, uint32_t * packed_out);
size_t dist_id_tracker_packed_size(const dist_id_tracker_t * t);
size_t dist_id_tracker_global_size(const dist_id_tracker_t * t);

/* ==== batched row engine (extension; SURVEY 8b "new batched entry points") ==
 * One PitmanYor driver + n_features slaves + an id tracker over a resident
 * table of rows -- the loop of examples/mixture/main.py:236-244 /
 * benchmarks/mixture.cc:104-115 with sampling, run for many rows per launch.
 *
 * Batch semantics: every row of a batch is scored against the
 * state at batch entry minus itself (exactly what remove_value leaves behind,
 * including group removal when the row was alone), draws with engine step
 * (draw_base + global row index + 1) of `seed_state`, and all moves are then
 * applied in row order.  A batch of one row is the reference's sequential
 * update. */
typedef struct dist_gibbs dist_gibbs_t;
dist_gibbs_t * dist_gibbs_create(float alpha, float d, int n_features,
                                 const dist_shared_t * shareds);
/* the same engine under the LowEntropy clustering model (generic driver
 * scores, mixture.hpp:124-141); dataset_size >= the total number of rows */
dist_gibbs_t * dist_gibbs_create_low_entropy(int dataset_size, int n_features,
                                             const dist_shared_t * shareds);
void dist_gibbs_destroy(dist_gibbs_t * g);

/* Rows that have no group yet: `empty_groups` empty groups, every row
 * unassigned (mixture.init(model) of a fresh mixture, examples/mixture/
 * main.py:222-224).  dist_gibbs_init_sequential then assigns rows
 * [row_begin, row_end) in order -- it must start at the first unassigned row
 * -- by the initialisation loop of examples/mixture/main.py: score every
 * group for the row (prior_only: with the clustering model alone, main.py:
 * 227-232; else with all features, main.py:265-270), sample, add; nothing is
 * removed; one engine step per row from *rng_state, which is advanced. */
int dist_gibbs_load_rows_unassigned(dist_gibbs_t * g, size_t n_rows,
                                    const uint32_t * const * values,
                                    int empty_groups, uint64_t row_offset);
int dist_gibbs_init_sequential(dist_gibbs_t * g, size_t row_begin,
                               size_t row_end, uint32_t * rng_state,
                               int prior_only);
/* Make n_rows rows resident.  values[f] -> n_rows words; assign_packed[i] in
 * [0, nonempty_groups); empty_groups >= 1 empty groups are appended
 * (mixture.hpp:152-162).  row_offset = global index of local row 0 (multi-GPU
 * shards).  The *_dev form takes device pointers and keeps using them. */
int dist_gibbs_load_rows(dist_gibbs_t * g, size_t n_rows,
                         const uint32_t * const * values,
                         const uint32_t * assign_packed, int nonempty_groups,
                         int empty_groups, uint64_t row_offset);
int dist_gibbs_load_rows_dev(dist_gibbs_t * g, size_t n_rows,
                             const uint32_t * const * values_dev,
                             uint32_t * assign_packed_dev, int nonempty_groups,
                             int empty_groups, uint64_t row_offset);
/* multi-GPU: the statistics were built from local rows only; add the other
 * shards' (dist_gibbs_stat_words() int32 words, all-reduced by the caller) */
size_t dist_gibbs_stat_words(const dist_gibbs_t * g);   /* (size_t)-1: failed, see dist_last_error */
int dist_gibbs_export_stats_dev(const dist_gibbs_t * g, int32_t * stats_dev);
int dist_gibbs_import_stats_dev(dist_gibbs_t * g, const int32_t * stats_dev);

/* one Gibbs pass over local rows [row_begin,row_end) in batches of
 * batch_rows, single GPU */
int dist_gibbs_sweep(dist_gibbs_t * g, size_t row_begin, size_t row_end,
                     size_t batch_rows, uint32_t seed_state,
                     uint64_t draw_base);
/* the reference's sequential chain (examples/mixture/main.py:236-244 over
 * mixture.hpp:73-122, 361-398: remove the row, score, sample, add -- a batch
 * of one row), advancing *rng_state one step per row.  Device-resident: one
 * workgroup walks the range, group creation and removal included. */
int dist_gibbs_sweep_sequential(dist_gibbs_t * g, size_t row_begin,
                                size_t row_end, uint32_t * rng_state);
/* M independent exact chains in ONE launch (BASELINE configs[3]: "8
 * independent chains"): engine i -- its own rows, statistics, id maps --
 * runs dist_gibbs_sweep_sequential over ITS rows [row_begin, row_end) with
 * rng_states[i], one workgroup per chain, side by side on the GPU; each
 * chain's result is exactly that of its own sequential call.  The engines
 * share one feature list (same kinds, any hyper-parameters) and are distinct;
 * up to two chains fit a compute unit (512 on an MI355X run concurrently). */
int dist_gibbs_sweep_sequential_many(dist_gibbs_t * const * engines, size_t m,
                                     size_t row_begin, size_t row_end,
                                     uint32_t * rng_states);
/* the same pass in phases, for callers that exchange statistics between
 * GPUs: sample -> delta -> [all-reduce delta] -> apply_delta ->
 * (ordered statistics: moves -> [all-gather] -> replay_ordered) -> finish.
 * delta is dist_gibbs_stat_words() int32 words of device memory and carries
 * the statistics that add over ranks (group sizes, DD/DPD/BB counts, GP count
 * and sum). */
int dist_gibbs_batch_sample(dist_gibbs_t * g, size_t row_begin, size_t row_end,
                            uint32_t seed_state, uint64_t draw_base);
int dist_gibbs_batch_delta_dev(dist_gibbs_t * g, int32_t * delta_dev);
int dist_gibbs_batch_apply_delta_dev(dist_gibbs_t * g,
                                     const int32_t * delta_dev);
int dist_gibbs_batch_apply_local(dist_gibbs_t * g);
/* "float_stats" = 1 (merged; opt-in, tolerance-level): the order-dependent
 * statistics -- NormalInverseChiSq's count / mean / count_times_variance
 * (nich.hpp:125-165), GammaPoisson's log_prod (gp.hpp:115,134) -- are updated
 * from binary64 SUMS per group (change of the count, of sum x, of sum x^2; of
 * log_prod) instead of being replayed row by row: equal to the running
 * updates to binary32 rounding, not bit for bit.  The sums add over ranks:
 * dist_gibbs_float_delta_words() doubles per image (0: not in this mode);
 * between dist_gibbs_batch_apply_delta_dev and dist_gibbs_batch_finish a
 * multi-rank caller takes its open batch's image, all-reduces it and hands it
 * back; dist_gibbs_sweep_sharded does so itself.  After every rank loaded
 * ITS rows: export, all-reduce, import (the import replaces the rank's own). */
size_t dist_gibbs_float_delta_words(const dist_gibbs_t * g);
int dist_gibbs_batch_float_delta_dev(dist_gibbs_t * g, double * delta_dev);
int dist_gibbs_batch_apply_float_delta_dev(dist_gibbs_t * g,
                                           const double * delta_dev);
int dist_gibbs_export_float_moments_dev(dist_gibbs_t * g, double * out_dev);
int dist_gibbs_import_float_moments_dev(dist_gibbs_t * g,
                                        const double * image_dev);
int dist_gibbs_batch_finish(dist_gibbs_t * g);
/* Order-dependent statistics -- all of NormalInverseChiSq's (Welford updates,
 * nich.hpp:125-165) and GammaPoisson's log_prod (gp.hpp:115,134) -- do not add
 * over ranks: they are replayed in global row order on every replica.
 * ordered_features: how many features carry such statistics.
 * batch_moves_dev: the open batch's moves in row order (slot indices of the
 * batch snapshot, identical on every replica); call after batch_delta_dev.
 * replay_ordered_dev: row i of the gathered list (rank order) leaves slot
 * old_slot[i] (NULL: additions only) and joins new_slot[i]; 0xFFFFFFFF in
 * new_slot marks padding; values_dev[f] -> n_rows words for every ordered
 * feature f (other entries may be NULL).  reset != 0 returns those statistics
 * to Group::init first (replay of the whole data set after load_rows). */
int dist_gibbs_ordered_features(const dist_gibbs_t * g, int * count_out);
int dist_gibbs_batch_moves_dev(dist_gibbs_t * g, uint32_t * old_slot_dev,
                               uint32_t * new_slot_dev);
int dist_gibbs_replay_ordered_dev(dist_gibbs_t * g,
                                  const uint32_t * old_slot_dev,
                                  const uint32_t * new_slot_dev,
                                  const uint32_t * const * values_dev,
                                  size_t n_rows, int reset);

/* ---- the library's own communicator ----------------------------------------
 * Optional: with it the whole multi-GPU sweep (sample -> delta -> all-reduce
 * -> apply -> finish, per sub-sweep) runs inside the library, the all-reduce
 * on the engine's own stream.  Two transports, chosen by the id:
 *   RCCL (dist_comm_unique_id): bound at run time (the librccl.so.1 already
 *     in the process, e.g. PyTorch's, else ROCm's); one process per GPU.
 *   host (dist_comm_unique_id_host): ranks that SHARE a GPU -- RCCL refuses
 *     two ranks on one device -- meet in a POSIX shared-memory segment and
 *     the all-reduce is staged through the host (drains the stream: for tests
 *     and single-GPU rehearsals of the multi-rank protocol).  It checks that
 *     all ranks issue the same collective and fails the call on every rank
 *     ("ranks diverged") instead of hanging when they do not, or when a peer
 *     does not arrive within DIST_COMM_TIMEOUT_S seconds (default 120).
 * Rank 0 makes the id and hands the 128 bytes to the other ranks by whatever
 * channel the application has (torch.distributed broadcast, MPI, a file);
 * every rank then calls dist_comm_create (collective).  Engines with
 * order-dependent statistics (NormalInverseChiSq, GammaPoisson's log_prod) are
 * refused by dist_gibbs_sweep_sharded: they exchange rows (see above), or
 * sums with "float_stats" = 1. */
typedef struct dist_comm dist_comm_t;
int dist_comm_available(void);                       /* 1 if RCCL can be bound */
int dist_comm_unique_id(uint8_t id_out[128]);
int dist_comm_unique_id_host(uint8_t id_out[128]);
dist_comm_t * dist_comm_create(const uint8_t id[128], int rank, int world);
void dist_comm_destroy(dist_comm_t * c);
int dist_comm_size(const dist_comm_t * c, int * rank_out, int * world_out);
/* in-place all-reduce of device memory on the calling thread's stream, waited
 * for: type 0 = int32, 1 = binary64; op 0 = sum, 1 = min (what the engines'
 * own exchanges use; for the application's set-up steps, e.g. the statistics
 * after every rank loaded its rows) */
int dist_comm_all_reduce_dev(dist_comm_t * c, void * data_dev, size_t count,
                             int type, int op);
/* n_batches sub-sweeps over the local rows in batches of batch_rows (ranks
 * whose shard is exhausted take part with empty batches: pass the same
 * n_batches on every rank).  Per sub-sweep ONE all-reduce of
 *   4 + min(bound, K0 + j * empty_groups) * (3 + dim)   int32 words
 * (K0: the group count the ranks' run began with, j: its batches so far --
 * the live part of the group set, not the bound buffers are sized by), or of
 *   4 + 3 * min(bound, K0 + j * empty_groups)
 * on value-partitioned ranks (below).  The 4 header words let the ranks tell
 * that one of them left the common run (dist_last_error: "ranks diverged";
 * the engine is unusable then) -- between two passes a rank may LOOK at its
 * engine (counts, assignments, groups, validate, statistics export, timers)
 * but not change it. */
int dist_gibbs_sweep_sharded(dist_gibbs_t * g, dist_comm_t * c,
                             size_t n_batches, size_t batch_rows,
                             uint32_t seed_state, uint64_t draw_base);
/* Value-partitioned ranks (one categorical feature: DirichletDiscrete,
 * DirichletProcessDiscrete): when the rows are placed so that no value has
 * rows on two ranks, a rank's rows only ever touch the cells counts[.][x] of
 * ITS values (dd.hpp:123-149, dpd.hpp:430-469) -- those cells never travel,
 * and what the ranks exchange per sub-sweep is the group sizes and the
 * per-group totals, 3 words per group (C2: 12 KB instead of 1.1 MB; C5: 98 KB
 * instead of 328 MB).  partition_by_value (collective, after load_rows and
 * the initial statistics exchange) checks the placement -- a value with rows
 * on two ranks fails the call on every rank -- and switches
 * dist_gibbs_sweep_sharded to that exchange.  From then on the cells of OTHER
 * ranks' values are stale here: entry points that read whole groups
 * (get_group, validate, export_stats, score_data) fail until gather_cells
 * (collective: one all-reduce of the owned cells) has made the replicas
 * whole again.  Results are those of the unpartitioned exchange, bit for
 * bit. */
int dist_gibbs_partition_by_value(dist_gibbs_t * g, dist_comm_t * c);
int dist_gibbs_gather_cells(dist_gibbs_t * g, dist_comm_t * c);
/* the exchanges of dist_gibbs_sweep_sharded since the last reset: out[0] =
 * all-reduces issued, out[1] = int32 words sent in all of them, out[2] = the
 * largest, out[3] = the last one (header included; does not close a run) */
int dist_gibbs_comm_volume(dist_gibbs_t * g, uint64_t out[4], int reset);

/* batch-semantics scores of one resident row (length written to *size_out;
 * scores_out needs dist_gibbs_group_count() floats) */
int dist_gibbs_row_scores(dist_gibbs_t * g, size_t row, float * scores_out,
                          size_t * size_out);
/* score_values extension: scores[r * ld + k] for rows [row_begin,row_end)
 * against the current state (no self-removal), device output; columns K..ld-1
 * are not written.  Refused while a batch is open (as dist_gibbs_row_scores);
 * launched in chunks of whole rows under the 1-D grid limit. */
int dist_gibbs_score_rows_dev(dist_gibbs_t * g, size_t row_begin,
                              size_t row_end, float * scores_dev, size_t ld);
/* Held-out rows: rows that are NOT in the table, scored against the current
 * state.  For query row q with values values[f][q]:
 *   scores[k], k in [0, dist_gibbs_group_count), empty groups included (they
 *     carry the new-group mass): the driver's score_value (clustering.hpp:
 *     195-208; under LowEntropy the generic MixtureDriver's, mixture.hpp:
 *     124-141) plus every slave's score_value in feature order (mixture.hpp:
 *     416-425) -- the arithmetic and order of dist_gibbs_score_rows_dev, with
 *     nothing removed first: a held-out row belongs to no group;
 *   logp[q] = log_sum_exp(scores) (random.cc:78-92): the maximum, the
 *     in-order float sum of fast_exp(scores[k] - max), fast_log(total) + max.
 *     Under PitmanYor the driver's scores are normalised and logp[q] is the
 *     log posterior predictive density of the row; under LowEntropy they are
 *     not, and *prior_total_out, log_sum_exp of the driver's scores alone, is
 *     what the caller subtracts;
 *   group[q]: mode 0 draws it by sample_from_scores_overwrite (random.hpp:
 *     361-366 over random.cc:94-106 and random.hpp:316-333) with engine step
 *     draw_base + q + 1 of seed_state, the batch's own convention, so that
 *     results do not depend on chunking or launch geometry; mode 1 takes the
 *     first index that attains the maximum.  Either way the GLOBAL group id,
 *     as dist_gibbs_assignments returns them.
 * values: F columns of n_rows 32-bit words (float bits for
 * NormalInverseChiSq), every feature observed.  logp, group and
 * prior_total_out may each be NULL.  A DirichletDiscrete value >= dim or a
 * BetaBernoulli value > 1 reads nothing out of bounds: the call fails with
 * dist_last_error() naming the first such row and its feature, and the
 * outputs are then unspecified.  A DirichletProcessDiscrete value the table
 * does not hold (>= its size, DIST_DPD_OTHER among them) is valid and scores
 * as OTHER (dpd.hpp:534-542).  A pure reader: rows, statistics, id maps,
 * caches and random state of the engine are left as they were; a run a sweep
 * left open is closed and stays resumable.  Refused while a batch is open and
 * on a value-partitioned rank whose cells are stale (dist_gibbs_gather_cells
 * first).  n_rows == 0 does nothing.  Returns when the work is done.  Memory:
 * O(n_rows + group count); no n_rows x groups matrix exists anywhere.
 * _dev: device pointers throughout (values_dev itself is a host array of F
 * device pointers), prior_total_out a host scalar.  The host form stages,
 * calls and downloads. */
int dist_gibbs_predict_dev(dist_gibbs_t * g, size_t n_rows,
                           const uint32_t * const * values_dev,
                           float * logp_dev, uint32_t * group_dev, int mode,
                           uint32_t seed_state, uint64_t draw_base,
                           float * prior_total_out);
int dist_gibbs_predict(dist_gibbs_t * g, size_t n_rows,
                       const uint32_t * const * values, float * logp_out,
                       uint32_t * group_out, int mode, uint32_t seed_state,
                       uint64_t draw_base, float * prior_total_out);
/* Held-out rows against M engines at once: the predictive averaged over the
 * members of an ensemble, e.g. the chains dist_gibbs_sweep_sequential_many
 * advances, each one posterior sample of the partition and, after
 * dist_gibbs_sample_hypers, of the hyper-parameters.  An extension: the
 * reference has no such member, only the folds reused here.  For query row q
 * and engine e in [0, m):
 *   w[e][q] = logp[q] of dist_gibbs_predict on engine e, bit for bit; under
 *     LowEntropy minus that engine's prior_total, one float subtraction (under
 *     PitmanYor nothing is subtracted);
 *   logp[q] = log_sum_exp(w[0..m)[q]) - fast_log((float)m): log (1/m) sum_e
 *     p(x_q | state_e), with log_sum_exp as random.cc:78-92 has it -- the
 *     maximum, the in-order float sum of fast_exp(w - max), fast_log(total) +
 *     max.  For m == 1 these are dist_gibbs_predict's bits (minus prior_total
 *     under LowEntropy).  A member value of -inf or NaN gives what that fold
 *     gives;
 *   member[q]: mode 0 draws the engine by sample_from_scores_overwrite
 *     (random.hpp:361-366) over w[.][q] with engine step draw_base + q + 1 of
 *     member_seed_state; mode 1 takes the first index that attains the
 *     maximum;
 *   group[q]: the group dist_gibbs_predict gives row q on engine member[q]
 *     with the same mode, seed_state and draw_base (mode 0: engine step
 *     draw_base + q + 1 of seed_state), as that engine's GLOBAL id.
 *   members_logp: the planes w, plane e at members_logp + e * members_ld
 *     (members_ld >= n_rows); prior_totals_out[e]: engine e's prior_total.
 * values: F columns of n_rows words, every feature observed.  Every output
 * may be NULL.  The engines are distinct and share one feature list (kinds
 * and dim) and one clustering model; hyper-parameters, group counts, rows
 * and id maps may all differ.  A pure reader of every engine under the rules
 * of dist_gibbs_predict: a run a sweep left open stays resumable, an open
 * batch or stale cells on any engine are refused, a value outside its domain
 * fails the call naming the first such row and its feature, a
 * DirichletProcessDiscrete value outside the table scores as OTHER.  m == 0
 * or n_rows == 0 does nothing.  Scratch: m x chunk words per plane, chunk the
 * most rows that keep a plane under 1 GiB and at most the first engine's
 * "debug.predict_chunk"; results do not depend on it.  One host wait per
 * call.
 * flags: DIST_PREDICT_MANY_DRAW_ALL draws the group in EVERY member and
 * selects afterwards, instead of drawing only in the chosen one (same bits;
 * the A/B partner of the default).
 * _dev: device pointers throughout (engines and values_dev are host arrays),
 * prior_totals_out a host array of m floats.  The host form stages, calls
 * and downloads. */
#define DIST_PREDICT_MANY_DRAW_ALL 1u
int dist_gibbs_predict_many_dev(dist_gibbs_t * const * engines, size_t m,
                                size_t n_rows,
                                const uint32_t * const * values_dev,
                                float * logp_dev, uint32_t * member_dev,
                                uint32_t * group_dev, int mode,
                                uint32_t seed_state,
                                uint32_t member_seed_state,
                                uint64_t draw_base, float * members_logp_dev,
                                size_t members_ld, float * prior_totals_out,
                                unsigned flags);
int dist_gibbs_predict_many(dist_gibbs_t * const * engines, size_t m,
                            size_t n_rows, const uint32_t * const * values,
                            float * logp_out, uint32_t * member_out,
                            uint32_t * group_out, int mode,
                            uint32_t seed_state, uint32_t member_seed_state,
                            uint64_t draw_base, float * members_logp_out,
                            size_t members_ld, float * prior_totals_out,
                            unsigned flags);

/* Held-out rows: co-assignment of row pairs over M engines, the similarity
 * behind search, de-duplication and consensus clustering across chains.  An
 * extension: the reference has no such member, only the pieces reused here.
 * For engine e in [0, m) and row a, scores[k], the maximum mx and total are
 * exactly dist_gibbs_predict's (scores_to_likelihoods, random.cc:94-103: the
 * maximum, the in-order float sum of fast_exp(scores[k] - mx)), k in [0,
 * dist_gibbs_group_count of e), empty groups included.  Then
 *   r_e,a[k] = fast_exp(scores[k] - mx) * (1.0f / total): one IEEE float
 *     division per row and one float multiply per group, subnormal results
 *     flushed to zero.  The normalisation is per engine, so LowEntropy needs
 *     nothing more (no prior_total);
 *   acc[a][b] = fmaf(r_e,a[k], r_e,b[k], acc[a][b]) from 0.0f: ONE chain per
 *     cell, engines ascending, k ascending within an engine; a the query row,
 *     b the target row;
 *   out[a * ld + b] = acc[a][b] / (float)m, IEEE division (ld >= n_t).
 * This is the probability that dist_gibbs_predict with mode 0 puts rows a and
 * b into the same slot when the engine is drawn uniformly and the two draws
 * are independent.  It is NOT the joint law in which a joining a group changes
 * b's predictive, and empty slots count as distinct groups: with several empty
 * groups the new-group mass divides among them.  Cells of a row whose logp is
 * not finite (DirichletProcessDiscrete OTHER with beta0 = 0) are unspecified.
 * values_t == NULL: the targets are the queries, n_t is ignored and the
 * result is symmetric bit for bit.  The engines are distinct and share one
 * feature list and one clustering model, as for dist_gibbs_predict_many, and
 * the calls are pure readers under its rules: a run a sweep left open stays
 * resumable, an open batch or stale cells on any engine are refused, a value
 * outside its domain fails the call naming the first such row and its feature
 * ("target row" for one of values_t).  m == 0, n_q == 0 or n_t == 0 does
 * nothing.  Scratch: the engines' responsibilities of a chunk of rows, k-major,
 * under 1 GiB; chunk at most the first engine's "debug.predict_chunk"; results
 * do not depend on it or on the launch geometry.  One host wait per call.
 * dist_gibbs_coassign is the m == 1 form.
 * dist_gibbs_responsibilities writes resp[k * ld + q] = r[k] of row q on
 * engine g (k-major, ld >= n_rows, dist_gibbs_group_count rows of it): the
 * group posterior of a held-out row, and the first phase of the calls above on
 * its own.
 * _dev: device pointers throughout (engines and values_*_dev are host
 * arrays).  The host forms stage, call and download. */
int dist_gibbs_coassign_many_dev(dist_gibbs_t * const * engines, size_t m,
                                 size_t n_q,
                                 const uint32_t * const * values_q_dev,
                                 size_t n_t,
                                 const uint32_t * const * values_t_dev,
                                 float * out_dev, size_t ld);
int dist_gibbs_coassign_many(dist_gibbs_t * const * engines, size_t m,
                             size_t n_q, const uint32_t * const * values_q,
                             size_t n_t, const uint32_t * const * values_t,
                             float * out, size_t ld);
int dist_gibbs_coassign_dev(dist_gibbs_t * g, size_t n_q,
                            const uint32_t * const * values_q_dev, size_t n_t,
                            const uint32_t * const * values_t_dev,
                            float * out_dev, size_t ld);
int dist_gibbs_coassign(dist_gibbs_t * g, size_t n_q,
                        const uint32_t * const * values_q, size_t n_t,
                        const uint32_t * const * values_t, float * out,
                        size_t ld);
int dist_gibbs_responsibilities_dev(dist_gibbs_t * g, size_t n_rows,
                                    const uint32_t * const * values_dev,
                                    float * resp_dev, size_t ld);
int dist_gibbs_responsibilities(dist_gibbs_t * g, size_t n_rows,
                                const uint32_t * const * values, float * resp,
                                size_t ld);

/* Held-out rows: per query, the k targets it is most likely co-assigned with
 * over M engines -- what search and de-duplication need of the matrix above,
 * without the matrix.  cell(a, b) is, bit for bit, the float that
 * dist_gibbs_coassign_many writes to out[a * ld + b] for the same engines and
 * rows (one fmaf chain per cell, engines ascending, slots ascending, then
 * / (float)m).
 *   Eligible targets of query a: every b in [0, n_t); with
 *     DIST_COASSIGN_EXCLUDE_SELF, b == a is left out.  The flag is legal only
 *     when values_t == NULL (the targets are the queries, n_t is ignored) and
 *     fails the call otherwise, as does any other flag bit.
 *   Order: by cell descending, and among bit-equal cells by b ascending.  Cells
 *     of specified rows are >= +0 and never NaN, so this is the descending
 *     order of key = ((uint64_t)bits(cell) << 32) | (0xFFFFFFFF - b); keys of
 *     distinct targets are distinct, so the result does not depend on tiles,
 *     chunks, launch geometry or "debug.predict_chunk".
 *   Output: for j < min(k, number of eligible targets), index_out[a * ld + j]
 *     is the j-th target and prob_out[a * ld + j] its cell; for larger j < k
 *     the entries are 0xFFFFFFFF and +0.0f (key 0, below every real key).
 *   Limits: ld >= k and k <= 128, otherwise the call fails; k == 0, m == 0,
 *     n_q == 0 or n_t == 0 does nothing; n_t <= 2^32 - 2.
 * Rows with non-finite logp (dist_gibbs_coassign_many leaves their cells
 * unspecified): a QUERY row with non-finite logp on any engine has an
 * unspecified result row; if ANY TARGET row has non-finite logp on any engine,
 * the whole call's result is unspecified (its cells may displace any row's
 * targets).  Engines, readers, errors and the one host wait are
 * dist_gibbs_coassign_many's.  Scratch: its planes, the running k keys of
 * every query (8 k n_q bytes) and the candidate keys of one launch, under
 * 1 GiB.  dist_gibbs_coassign_topk is the m == 1 form.
 * _dev: device pointers throughout (engines and values_*_dev are host
 * arrays).  The host forms stage, call and download. */
#define DIST_COASSIGN_EXCLUDE_SELF 1u
int dist_gibbs_coassign_topk_many_dev(dist_gibbs_t * const * engines, size_t m,
                                      size_t n_q,
                                      const uint32_t * const * values_q_dev,
                                      size_t n_t,
                                      const uint32_t * const * values_t_dev,
                                      size_t k, unsigned flags,
                                      uint32_t * index_out_dev,
                                      float * prob_out_dev, size_t ld);
int dist_gibbs_coassign_topk_many(dist_gibbs_t * const * engines, size_t m,
                                  size_t n_q,
                                  const uint32_t * const * values_q,
                                  size_t n_t,
                                  const uint32_t * const * values_t, size_t k,
                                  unsigned flags, uint32_t * index_out,
                                  float * prob_out, size_t ld);
int dist_gibbs_coassign_topk_dev(dist_gibbs_t * g, size_t n_q,
                                 const uint32_t * const * values_q_dev,
                                 size_t n_t,
                                 const uint32_t * const * values_t_dev,
                                 size_t k, unsigned flags,
                                 uint32_t * index_out_dev,
                                 float * prob_out_dev, size_t ld);
int dist_gibbs_coassign_topk(dist_gibbs_t * g, size_t n_q,
                             const uint32_t * const * values_q, size_t n_t,
                             const uint32_t * const * values_t, size_t k,
                             unsigned flags, uint32_t * index_out,
                             float * prob_out, size_t ld);

/* Held-out rows: one feature's predictive given the others.  For query row q,
 * a target feature t, candidate words cand[0..C) for t and a mask observed[q]
 * (bit f set: feature f of row q is observed; bit t is ignored; observed ==
 * NULL: every other feature is observed):
 *   scores_c[k], k in [0, dist_gibbs_group_count), empty groups included: the
 *     driver's score_value as in dist_gibbs_predict (clustering.hpp:195-208;
 *     mixture.hpp:124-141 under LowEntropy), then in feature order
 *     (mixture.hpp:416-425) every OBSERVED feature's score_value with the
 *     row's value and, at position t, the target's with cand[c].  An
 *     unobserved feature contributes nothing, not even a +0;
 *   joint[q * C + c] = log_sum_exp(scores_c) (random.cc:78-92): the maximum,
 *     the in-order float sum of fast_exp(s - max), fast_log(total) + max.
 *     With every other feature observed these are the bits dist_gibbs_predict
 *     returns as logp for the row completed with cand[c];
 *   base[q] = log_sum_exp of the same fold with the target left out: the log
 *     marginal of the observed cells; with nothing observed, predict's
 *     *prior_total_out, bit for bit;
 *   the conditional log p(x_t = cand[c] | observed cells) is joint - base,
 *     which the caller forms; the driver's unnormalised mass under LowEntropy
 *     cancels in it, so no prior_total is returned;
 *   choice[q], an INDEX into the candidates: mode 0 draws it by
 *     sample_from_scores_overwrite (random.hpp:361-366 over random.cc:94-106
 *     and random.hpp:316-333) over joint[q][0..C) with engine step
 *     draw_base + q + 1 of seed_state, the batch's own convention, so that
 *     results do not depend on chunking or launch geometry; mode 1 takes the
 *     first index of maximal joint.  joint itself is not overwritten.
 * candidates: a HOST array of n_candidates words in both forms (counts, or
 * float bits for NormalInverseChiSq), validated before any launch: a
 * DirichletDiscrete word >= dim or a BetaBernoulli word > 1 fails and names
 * the candidate's index; a DirichletProcessDiscrete word the table does not
 * hold scores as OTHER (dpd.hpp:534-542).  candidates == NULL means the whole
 * domain: 0 .. dim-1 (DD), 0, 1 (BB), 0 .. dim-1 then DIST_DPD_OTHER (DPD);
 * the other kinds need a list.  C is the length of the list in use.
 * values: F columns of n_rows words; words in unobserved cells are never
 * interpreted and the target's column pointer may be NULL.  An OBSERVED
 * DirichletDiscrete value >= dim or BetaBernoulli value > 1 reads nothing out
 * of bounds: the call fails naming the first such row and its feature, and
 * the outputs are then unspecified.  joint, base and choice may each be NULL;
 * choice without joint keeps joint in engine scratch, the rows chunked so that
 * it stays under 1 GiB (and under "debug.predict_chunk" rows).
 * flags: DIST_PREDICT_FEATURE_RECOMPUTE scores every (row, candidate) pair
 * from scratch instead of evaluating a row's candidate-independent part once
 * (the same bits; for comparison).
 * A pure reader under the rules of dist_gibbs_predict: nothing in the engine
 * changes, refused while a batch is open and on a value-partitioned rank
 * whose cells are stale; n_rows == 0 does nothing.  Returns when the work is
 * done.
 * _dev: values_dev is a host array of F device pointers; observed_dev, joint,
 * base and choice are device pointers.  The host form stages, calls and
 * downloads. */
#define DIST_PREDICT_FEATURE_RECOMPUTE 1u
int dist_gibbs_predict_feature_dev(dist_gibbs_t * g, size_t n_rows,
                                   const uint32_t * const * values_dev,
                                   const uint32_t * observed_dev, int target,
                                   const uint32_t * candidates,
                                   size_t n_candidates, float * joint_dev,
                                   float * base_dev, uint32_t * choice_dev,
                                   int mode, uint32_t seed_state,
                                   uint64_t draw_base, unsigned flags);
int dist_gibbs_predict_feature(dist_gibbs_t * g, size_t n_rows,
                               const uint32_t * const * values,
                               const uint32_t * observed, int target,
                               const uint32_t * candidates,
                               size_t n_candidates, float * joint_out,
                               float * base_out, uint32_t * choice_out,
                               int mode, uint32_t seed_state,
                               uint64_t draw_base, unsigned flags);
/* Held-out rows: one feature's predictive given the others, averaged over the
 * members of an ensemble of M engines (dist_gibbs_predict_many's ensembles).
 * An extension: the reference has no such member, only the folds reused here.
 * For query row q, target t, candidate words cand[0..C), mask observed[q]
 * (the bits of dist_gibbs_predict_feature: bit t is ignored, observed == NULL
 * means every other feature is observed) and engine e in [0, m):
 *   wj[e][q * C + c] = joint[q * C + c] of dist_gibbs_predict_feature on
 *     engine e, bit for bit; under LowEntropy minus that engine's prior_total,
 *     one float subtraction (under PitmanYor nothing is subtracted);
 *   wb[e][q] = the same for base[q];
 *   joint[q * C + c] = log_sum_exp(wj[0..m)[q * C + c]) - fast_log((float)m)
 *     and base[q] = log_sum_exp(wb[0..m)[q]) - fast_log((float)m), with
 *     log_sum_exp as random.cc:78-92 has it -- the maximum, the in-order float
 *     sum of fast_exp(w - max), fast_log(total) + max: the logs of
 *     (1/m) sum_e p(x_t = cand[c], x_obs | e) and (1/m) sum_e p(x_obs | e).
 *     For m == 1 these are dist_gibbs_predict_feature's bits (minus
 *     prior_total under LowEntropy);
 *   the ensemble's conditional log p(x_t = cand[c] | x_obs) is joint - base,
 *     which the caller forms: a RATIO OF AVERAGES,
 *       sum_e p(x_t, x_obs | e) / sum_e p(x_obs | e),
 *     the members' conditionals weighted by how well each explains the
 *     observed cells (p(e | x_obs) is proportional to p(x_obs | e)).  It is
 *     not the mean over e of the members' joint - base, which weights every
 *     member alike whatever the row shows.  Under LowEntropy each member's
 *     unnormalised driver mass is its own and no longer cancels in the ratio,
 *     hence the subtraction above;
 *   choice[q], an INDEX into the candidates: mode 0 draws it by
 *     sample_from_scores_overwrite (random.hpp:361-366) over the FOLDED
 *     joint[q][0..C) with engine step draw_base + q + 1 of seed_state; mode 1
 *     takes the first index of maximal folded joint;
 *   member[q]: the engine drawn from wb[.][q], the posterior over the members
 *     given the observed cells: mode 0 by sample_from_scores_overwrite with
 *     engine step draw_base + q + 1 of member_seed_state, mode 1 the first
 *     maximum.  (member, then dist_gibbs_sample_rows on that engine, composes
 *     an ensemble draw of the missing cells.)
 *   members_joint: the planes wj, plane e at members_joint + e *
 *     members_joint_ld (members_joint_ld >= n_rows * C); members_base: the
 *     planes wb, plane e at members_base + e * members_base_ld
 *     (members_base_ld >= n_rows); prior_totals_out[e]: engine e's
 *     prior_total, a HOST array of m floats.
 * Every output may be NULL.  When neither joint, choice nor members_joint is
 * asked for, only the base chain runs.
 * candidates: a HOST array in both forms, validated once, before any launch,
 * against the shared feature list by dist_gibbs_predict_feature's rules (a
 * DirichletDiscrete word >= dim or a BetaBernoulli word > 1 fails naming the
 * candidate's index, a DirichletProcessDiscrete word outside the table is
 * OTHER, NULL is the whole domain of a DD, BB or DPD target).  An observed
 * value outside its domain fails the call naming the first such row and its
 * feature; words in unobserved cells are never read; the target's column may
 * be NULL.  The engines are distinct and share one feature list (kinds and
 * dim) and one clustering model, at most 65535 of them.  A pure reader of
 * every engine under dist_gibbs_predict_many's rules: a run a sweep left open
 * stays resumable, an open batch or stale cells on any engine are refused.
 * m == 0 or n_rows == 0 does nothing.  flags must be 0.  Scratch: m x chunk x
 * C words for wj unless members_joint is given, m x chunk for wb unless
 * members_base is, chunk x C for joint when choice is asked without it; chunk
 * keeps m x chunk x C words under 1 GiB and is at most the first engine's
 * "debug.predict_chunk"; results do not depend on it or on launch geometry.
 * One host wait per call.
 * _dev: device pointers throughout; engines, values_dev (F device pointers),
 * candidates and prior_totals_out are host arrays.  The host form stages,
 * calls and downloads. */
int dist_gibbs_predict_feature_many_dev(
    dist_gibbs_t * const * engines, size_t m, size_t n_rows,
    const uint32_t * const * values_dev, const uint32_t * observed_dev,
    int target, const uint32_t * candidates, size_t n_candidates,
    float * joint_dev, float * base_dev, uint32_t * choice_dev,
    uint32_t * member_dev, int mode, uint32_t seed_state,
    uint32_t member_seed_state, uint64_t draw_base, float * members_joint_dev,
    size_t members_joint_ld, float * members_base_dev, size_t members_base_ld,
    float * prior_totals_out, unsigned flags);
int dist_gibbs_predict_feature_many(
    dist_gibbs_t * const * engines, size_t m, size_t n_rows,
    const uint32_t * const * values, const uint32_t * observed, int target,
    const uint32_t * candidates, size_t n_candidates, float * joint_out,
    float * base_out, uint32_t * choice_out, uint32_t * member_out, int mode,
    uint32_t seed_state, uint32_t member_seed_state, uint64_t draw_base,
    float * members_joint_out, size_t members_joint_ld,
    float * members_base_out, size_t members_base_ld,
    float * prior_totals_out, unsigned flags);

/* Held-out rows: whole rows and missing cells drawn from the mixture.  Per
 * query row q with mask observed[q] (bit f set: feature f of row q is
 * observed; bits >= F are ignored; observed == NULL: nothing is observed):
 *   scores[k], k in [0, dist_gibbs_group_count), empty groups included: the
 *     driver's score_value as in dist_gibbs_predict, then in feature order
 *     (mixture.hpp:416-425) every OBSERVED feature's score_value with the
 *     row's value -- dist_gibbs_predict_feature's `base` fold;
 *   group[q], a global id: sample_from_scores_overwrite (random.hpp:361-366)
 *     over them with engine step draw_base + q + 1 of seed_state.  With every
 *     feature observed it is dist_gibbs_predict's mode-0 group, bit for bit;
 *   cell (q, f) of every feature that is NOT observed: a draw from group[q]'s
 *     posterior predictive, Group::sample_value (dd.hpp:188-199,
 *     bb.hpp:154-160, gp.hpp:166-172, nich.hpp:204-210, bnb.hpp:168-174,
 *     dpd.hpp:275-305) as dist_group_sample_value defines it, keyed by
 *     (seed_state, draw_base + q, f); an empty group gives prior-predictive
 *     cells.  Observed cells are returned as given.
 * Results do not depend on chunking or launch geometry; calls over disjoint
 * [draw_base, draw_base + n_rows) ranges draw disjoint streams.
 * values: F columns of n_rows words, NULL altogether when observed is NULL; a
 * single column may be NULL for a feature no row observes.  Words in
 * unobserved cells are never read.  An observed DirichletDiscrete value >= dim
 * or BetaBernoulli value > 1 (or an observed cell of a NULL column) fails the
 * call naming the first such row and its feature; a DirichletProcessDiscrete
 * value the table does not hold scores as OTHER.  out: F columns of n_rows
 * words; out[f] may be values[f] (completion in place: only the unobserved
 * cells are written).  group may be NULL.  A cell whose bounded rejection loop
 * ran out of tries (NaN hyper-parameters) fails the call naming the first.
 * A pure reader under the rules of dist_gibbs_predict: nothing in the engine
 * changes, refused while a batch is open and on a value-partitioned rank whose
 * cells are stale; n_rows == 0 does nothing; at most "debug.predict_chunk"
 * rows per launch.  Returns when the work is done.
 * _dev: values_dev and out_dev are host arrays of F device pointers;
 * observed_dev and group_dev are device pointers.  The host form stages,
 * calls and downloads. */
int dist_gibbs_sample_rows_dev(dist_gibbs_t * g, size_t n_rows,
                               const uint32_t * const * values_dev,
                               const uint32_t * observed_dev,
                               uint32_t * const * out_dev,
                               uint32_t * group_dev, uint32_t seed_state,
                               uint64_t draw_base);
int dist_gibbs_sample_rows(dist_gibbs_t * g, size_t n_rows,
                           const uint32_t * const * values,
                           const uint32_t * observed, uint32_t * const * out,
                           uint32_t * group_out, uint32_t seed_state,
                           uint64_t draw_base);

/* Held-out rows: whole rows and missing cells drawn from an ensemble of m
 * engines -- a state first, then a group in that state, then the cells.  An
 * extension: the reference has no such member, only the folds reused here.
 * For query row q with mask observed[q] (dist_gibbs_sample_rows' bits;
 * observed == NULL: nothing is observed, what an all-zero mask gives) and
 * engine e in [0, m):
 *   wb[e][q] = log_sum_exp (random.cc:78-92) of dist_gibbs_sample_rows'
 *     scores[k] of row q on engine e: the fold dist_gibbs_predict_feature
 *     calls `base` and dist_gibbs_predict_feature_many members_base, bit for
 *     bit; under LowEntropy minus that engine's prior_total, one float
 *     subtraction.  With every feature observed it is
 *     dist_gibbs_predict_many's members_logp;
 *   base[q] = log_sum_exp(wb[0..m)[q]) - fast_log((float)m): the log of
 *     (1/m) sum_e p(x_obs | e), as dist_gibbs_predict_feature_many folds it;
 *   member[q]: the engine drawn from wb[.][q], the posterior over the members
 *     given the observed cells, by sample_from_scores_overwrite
 *     (random.hpp:361-366) with engine step draw_base + q + 1 of
 *     member_seed_state: dist_gibbs_predict_feature_many's mode-0 member for
 *     equal arguments;
 *   group[q] and every unobserved cell (q, f): what dist_gibbs_sample_rows on
 *     engine member[q] gives for row q of the same call (same values,
 *     observed, seed_state, draw_base) -- the group, that engine's global id,
 *     with engine step draw_base + q + 1 of seed_state, the cells
 *     (Group::sample_value, dd.hpp:188-199, bb.hpp:154-160, gp.hpp:166-172,
 *     nich.hpp:204-210, bnb.hpp:168-174, dpd.hpp:275-305) keyed by
 *     (seed_state, draw_base + q, f) on the drawn group's statistics.
 *     Observed cells are returned as given.
 * For m == 1 these are dist_gibbs_sample_rows' bits.  Results do not depend
 * on chunking or launch geometry.
 * values, observed, out: dist_gibbs_sample_rows' conventions and failures (an
 * observed value outside its domain, a cell whose bounded loop ran out: each
 * names the first such row and its feature, over all members); out[f] may be
 * values[f] (completion in place).  group, member and base may be NULL.  The
 * engines are distinct and share one feature list (kinds and dim) and one
 * clustering model, at most 65535 of them.  A pure reader of every engine
 * under dist_gibbs_predict_many's rules: a run a sweep left open stays
 * resumable, an open batch or stale cells on any engine are refused.  m == 0
 * or n_rows == 0 does nothing.  flags must be 0.  Scratch: m x chunk words for
 * wb (chunk keeps them under 1 GiB and is at most the first engine's
 * "debug.predict_chunk").  One host wait per call.
 * _dev: engines, values_dev and out_dev (F device pointers each) are host
 * arrays; observed_dev, group_dev, member_dev and base_dev are device
 * pointers.  The host form stages, calls and downloads. */
int dist_gibbs_sample_rows_many_dev(
    dist_gibbs_t * const * engines, size_t m, size_t n_rows,
    const uint32_t * const * values_dev, const uint32_t * observed_dev,
    uint32_t * const * out_dev, uint32_t * group_dev, uint32_t * member_dev,
    float * base_dev, uint32_t seed_state, uint32_t member_seed_state,
    uint64_t draw_base, unsigned flags);
int dist_gibbs_sample_rows_many(
    dist_gibbs_t * const * engines, size_t m, size_t n_rows,
    const uint32_t * const * values, const uint32_t * observed,
    uint32_t * const * out, uint32_t * group_out, uint32_t * member_out,
    float * base_out, uint32_t seed_state, uint32_t member_seed_state,
    uint64_t draw_base, unsigned flags);

/* Held-out rows: the log marginals of S feature subsets per row, on one
 * engine and averaged over the members of an ensemble of m engines
 * (dist_gibbs_predict_many's ensembles).  An extension: the reference has no
 * such member, only the folds reused here.  masks: a HOST array of n_masks
 * >= 1 words shared by all rows, bit f of masks[s] set when subset s names
 * feature f; duplicates and 0 are allowed.  For query row q, subset s and
 * engine e in [0, m):
 *   scores[k], k in [0, dist_gibbs_group_count), empty groups included: the
 *     driver's score_value as in dist_gibbs_predict, then in feature order
 *     (mixture.hpp:416-425) the score_value of every feature NAMED by masks[s]
 *     with the row's value; an unnamed feature contributes nothing --
 *     dist_gibbs_predict_feature's `base` fold with the mask per subset
 *     instead of per row;
 *   w[e][q * n_masks + s] = log_sum_exp(scores) (random.cc:78-92); under
 *     LowEntropy minus that engine's prior_total, one float subtraction (under
 *     PitmanYor nothing is subtracted).  For any target outside masks[s] it is
 *     dist_gibbs_predict_feature's base under the row mask masks[s], bit for
 *     bit (minus prior_total under LowEntropy); for the mask of all features
 *     dist_gibbs_predict's logp, for mask 0 its prior_total (under LowEntropy
 *     x - x);
 *   dist_gibbs_marginals: logp[q * n_masks + s] = w[0][q * n_masks + s], one
 *     engine and no fold;
 *   dist_gibbs_marginals_many: logp[q * n_masks + s] =
 *     log_sum_exp(w[0..m)[q * n_masks + s]) - fast_log((float)m), with
 *     log_sum_exp as random.cc:78-92 has it -- the maximum, the in-order float
 *     sum of fast_exp(w - max), fast_log(total) + max: the log of
 *     (1/m) sum_e p(x_S | e), as dist_gibbs_predict_feature_many folds base;
 *   members_logp: the planes w, plane e at members_logp + e * members_ld
 *     (members_ld >= n_rows * n_masks); prior_totals_out[e]: engine e's
 *     prior_total, a HOST array of m floats.
 * logp, members_logp and prior_totals_out may be NULL.
 * values: F columns of n_rows words; a column may be NULL for a feature no
 * mask names, and words of such features are never read.  A mask with a bit
 * >= F, or one that names a feature whose column is NULL, fails before any
 * launch naming the mask's index.  A DirichletDiscrete value >= dim or a
 * BetaBernoulli value > 1 under a NAMED feature fails the call naming the
 * first such row and its feature; a DirichletProcessDiscrete value the table
 * does not hold scores as OTHER.  The engines are distinct and share one
 * feature list (kinds and dim) and one clustering model, at most 65535 of
 * them.  A pure reader of every engine under dist_gibbs_predict_many's rules:
 * a run a sweep left open stays resumable, an open batch or stale cells on
 * any engine are refused.  Scratch: m x chunk x n_masks floats for w unless
 * members_logp is given; chunk keeps them under 1 GiB and is at most the
 * first engine's "debug.predict_chunk"; results do not depend on it or on
 * launch geometry.  One host wait per call.
 * _dev: device pointers throughout; engines, values_dev (F device pointers),
 * masks and prior_totals_out are host arrays.  The host form stages, calls
 * and downloads. */
int dist_gibbs_marginals_dev(dist_gibbs_t * g, size_t n_rows,
                             const uint32_t * const * values_dev,
                             const uint32_t * masks, size_t n_masks,
                             float * logp_dev);
int dist_gibbs_marginals(dist_gibbs_t * g, size_t n_rows,
                         const uint32_t * const * values,
                         const uint32_t * masks, size_t n_masks,
                         float * logp_out);
int dist_gibbs_marginals_many_dev(
    dist_gibbs_t * const * engines, size_t m, size_t n_rows,
    const uint32_t * const * values_dev, const uint32_t * masks,
    size_t n_masks, float * logp_dev, float * members_logp_dev,
    size_t members_ld, float * prior_totals_out);
int dist_gibbs_marginals_many(
    dist_gibbs_t * const * engines, size_t m, size_t n_rows,
    const uint32_t * const * values, const uint32_t * masks, size_t n_masks,
    float * logp_out, float * members_logp_out, size_t members_ld,
    float * prior_totals_out);

/* Which columns depend on each other: the mutual information of every feature
 * pair and the entropy of every feature under the predictive of one engine or
 * of an ensemble of m engines, estimated from n_samples rows drawn from it.
 * An extension: the reference has no such member.  Per chunk of rows, on the
 * device:
 *   the rows are those dist_gibbs_sample_rows_many draws with nothing
 *     observed for the same seed_state, member_seed_state and draw_base;
 *   L = dist_gibbs_marginals_many's logp of them (dist_gibbs_relate:
 *     dist_gibbs_marginals', one engine and no fold) under the masks {i}
 *     (i < F) and {i, j} (i < j);
 *   per pair, in double, with
 *     d_q = (double)L_ij[q] - (double)L_i[q] - (double)L_j[q] and c the d of
 *     the call's first row: sum_q (d_q - c) and sum_q (d_q - c)^2 -- shifted,
 *     so that the variance does not cancel where |mean| is many standard
 *     deviations; per feature the same of -(double)L_i[q].  sum d and sum d^2
 *     are formed from them on the host.  No floating-point atomics: a fixed
 *     tree per chunk and an in-order add over the chunks, so equal calls give
 *     equal bits.
 * mi_out[i * F + j] = mi_out[j * F + i] = the mean of d; mi_out[i * F + i] the
 * entropy estimate of feature i (the differential entropy of a
 * NormalInverseChiSq feature); stderr_out the square root of (sample variance
 * / n_samples), +inf for n_samples == 1.  Both are HOST arrays of F * F
 * doubles and may be NULL; moments_out, a HOST array of F * F * 2 doubles or
 * NULL, takes the sums themselves, cell (i, j) at [(i * F + j) * 2]: sum d,
 * then sum d^2 (what a caller pools over calls of disjoint draw_base ranges).
 * n_samples == 0 fails.  A drawn row whose L is not
 * finite makes the cells it enters NaN.  Conditional variants are composed by
 * the caller from dist_gibbs_sample_rows_many and dist_gibbs_marginals_many.
 * The engines: dist_gibbs_marginals_many's rules.  One host wait per call. */
int dist_gibbs_relate(dist_gibbs_t * g, size_t n_samples, uint32_t seed_state,
                      uint32_t member_seed_state, uint64_t draw_base,
                      double * mi_out, double * stderr_out,
                      double * moments_out);
int dist_gibbs_relate_many(dist_gibbs_t * const * engines, size_t m,
                           size_t n_samples, uint32_t seed_state,
                           uint32_t member_seed_state, uint64_t draw_base,
                           double * mi_out, double * stderr_out,
                           double * moments_out);

/* What M chains say about their RESIDENT rows: the agreement of P partitions
 * of the same n_rows rows, and the co-assignment of chosen resident rows.  An
 * extension: the reference has no such member.
 * The first m partitions are the resident assignments of m engines -- row i of
 * every engine is the same datum, which the caller vouches for --, the other x
 * are caller-supplied label columns (a ground truth, an earlier
 * dist_gibbs_assignments).  For partitions a, b let
 *   n_gh = #{i : label_a[i] = g and label_b[i] = h}.
 * On the device, and nothing else:
 *   sq[a * P + b] = sum_{g,h} n_gh^2: uint64, both triangles written, the
 *     diagonal sum_g n_g^2.  Integers: exact in any order.
 *   nlogn[a * P + b] = sum_{g,h : n_gh > 0} n_gh * log(n_gh): binary64 with the
 *     platform's log, same shape.  NULL skips all of its work.  No
 *     floating-point atomics: a cell is taken once, by its first row in the
 *     stable order by a's label, partials are added in a fixed order, so equal
 *     calls give equal bits.
 * Rand and adjusted Rand indices, Binder's distance, the variation of
 * information and the least-squares (Dahl 2006) consensus among the m samples
 * are host arithmetic on these two matrices (the Python package has them).
 * dist_partition_agreement_dev: labels_dev a HOST array of p DEVICE pointers
 * to n_rows words each, n_labels[a] an exclusive bound on partition a's
 * labels, sq_out / nlogn_out HOST arrays of p * p entries.  No engine is
 * involved; it needs only a HIP device.  dist_partition_agreement stages host
 * columns, calls and downloads.
 * dist_gibbs_partition_agreement_many: partitions 0 .. m - 1 are the engines'
 * assignments, then the x extra columns of n_rows words.  The engines are read
 * under dist_gibbs_assignments' rules: a run a sweep left open stays
 * resumable, value-sorted batches' assignments are flushed to row order, an
 * open batch is refused.  Their labels -- global group ids, which grow without
 * bound over a run -- are translated to packed indices on the device, so that
 * an engine's bins are its dist_gibbs_group_count.
 * dist_gibbs_partition_agreement is the m == 1 form.
 * Bin limit: a partition may have at most 18 432 labels (n_labels, or an
 * engine's group count): one uint32 count and one uint32 first-row word per
 * label in 144 KiB of LDS.
 * dist_gibbs_coassign_resident_many: out[i * ld + j] = float(c) / float(m), c
 * the number of engines in which resident rows rows_a[i] and rows_b[j] carry
 * the same group id (ld >= nb): the posterior similarity of chosen resident
 * rows.  rows_b == NULL: rows_a, nb is ignored, the result is its own
 * transpose and its diagonal 1.  dist_gibbs_coassign_resident: m == 1.
 * Refused, before any launch unless noted: engines of unequal
 * dist_gibbs_row_count, or n_rows that differs from it; an engine with
 * unassigned rows (dist_gibbs_load_rows_unassigned not yet initialised
 * through), naming the engine; the same engine twice; n_labels[a] above the
 * bin limit, naming the partition; n_rows >= 2^31 (a row index travels through
 * the sort doubled); a row index >= the engines' row count in rows_a / rows_b
 * (the _dev form finds it by a kernel, which reads nothing there); a label >=
 * n_labels[a] -- found by the first kernel, before anything reads a label as
 * an index: the call fails naming the partition and the first such row, and
 * the outputs are not written.  p == 0, m + x == 0 or n_rows == 0 does
 * nothing.  Scratch is allocated per call: the order of the rows (n_rows
 * words), one translated column, the sort's counters, p * p results.  Two
 * host waits per agreement call, one per co-assignment call.
 * _dev: label columns, row indices and out are device pointers (the arrays of
 * pointers, n_labels, sq_out and nlogn_out stay host arrays). */
int dist_partition_agreement_dev(size_t n_rows, size_t p,
                                 const uint32_t * const * labels_dev,
                                 const uint32_t * n_labels, uint64_t * sq_out,
                                 double * nlogn_out);
int dist_partition_agreement(size_t n_rows, size_t p,
                             const uint32_t * const * labels,
                             const uint32_t * n_labels, uint64_t * sq_out,
                             double * nlogn_out);
int dist_gibbs_partition_agreement_many_dev(
    dist_gibbs_t * const * engines, size_t m, size_t n_rows,
    const uint32_t * const * extra_labels_dev, size_t x,
    const uint32_t * extra_n_labels, uint64_t * sq_out, double * nlogn_out);
int dist_gibbs_partition_agreement_many(
    dist_gibbs_t * const * engines, size_t m, size_t n_rows,
    const uint32_t * const * extra_labels, size_t x,
    const uint32_t * extra_n_labels, uint64_t * sq_out, double * nlogn_out);
int dist_gibbs_partition_agreement(dist_gibbs_t * g, size_t n_rows,
                                   const uint32_t * const * extra_labels,
                                   size_t x, const uint32_t * extra_n_labels,
                                   uint64_t * sq_out, double * nlogn_out);
int dist_gibbs_coassign_resident_many_dev(
    dist_gibbs_t * const * engines, size_t m, const uint32_t * rows_a_dev,
    size_t na, const uint32_t * rows_b_dev, size_t nb, float * out_dev,
    size_t ld);
int dist_gibbs_coassign_resident_many(
    dist_gibbs_t * const * engines, size_t m, const uint32_t * rows_a,
    size_t na, const uint32_t * rows_b, size_t nb, float * out, size_t ld);
int dist_gibbs_coassign_resident_dev(dist_gibbs_t * g,
                                     const uint32_t * rows_a_dev, size_t na,
                                     const uint32_t * rows_b_dev, size_t nb,
                                     float * out_dev, size_t ld);
int dist_gibbs_coassign_resident(dist_gibbs_t * g, const uint32_t * rows_a,
                                 size_t na, const uint32_t * rows_b, size_t nb,
                                 float * out, size_t ld);

/* Which rows of the table are most like this one: per query the k RESIDENT
 * rows b of [row_begin, row_end) it is most co-assigned with over m engines
 * that hold the same rows in the same order, without the [n_q, N] matrix.
 * Two kinds of query, one target set, one order and one fill.
 * dist_gibbs_search_resident_many: queries are held-out rows, values[f][q] as
 * dist_gibbs_coassign_many takes them.  With r_e,q[k] bit for bit
 * dist_gibbs_responsibilities' value and slot_e(b) the packed index of the
 * group resident row b has in engine e (dist_gibbs_global_to_packed of its
 * assignment),
 *     acc = 0.0f; engines ascending: acc = acc + r_e,q[slot_e(b)]
 *     cell(q, b) = acc / (float)m            (IEEE division)
 * one chain of binary32 adds.  It is the probability that dist_gibbs_predict's
 * draw puts q into the slot b occupies, the engine drawn uniformly.  It is NOT
 * normalised over b (it sums to the mean group size), and rows that share a
 * group in every engine have bit-equal cells: with one engine a query's k
 * targets are the k lowest-indexed rows of its best group, and it takes
 * several chains to tell rows apart.  A query whose logp is not finite on some
 * engine has an unspecified result row; targets are never scored.
 * dist_gibbs_coassign_resident_topk_many: queries are resident rows rows[a].
 *     cell(a, b) = (float)c / (float)m
 * c the engines in which rows[a] and b carry the same group id: bit for bit
 * dist_gibbs_coassign_resident_many's cell.  With DIST_COASSIGN_EXCLUDE_SELF
 * b == rows[a] is left out -- the row, not the position: duplicate queries are
 * legal.  The flag is legal only here.
 * Order and fill are dist_gibbs_coassign_topk_many's: targets by cell
 * descending and among bit-equal cells by b ascending, the descending order of
 * key = (uint64(bits(cell)) << 32) | (0xFFFFFFFF - b); where fewer than k
 * targets exist the rest is index 0xFFFFFFFF, prob +0.0f.  index_out[q * ld +
 * j] is the row's index in the engine, not its offset in the range.
 * 1 <= k <= 128, ld >= k, row_end <= 2^32 - 1.  The result does not depend on
 * slices, chunks or launch geometry.  m == 0, n_q == 0 or k == 0 does nothing;
 * an empty range writes the fill.
 * Refused: what dist_gibbs_coassign_resident_many refuses of the engines
 * (unequal row counts, unassigned rows, the same engine twice, an open
 * batch); for held-out queries also what dist_gibbs_coassign_many refuses
 * (feature lists or clustering models that differ, stale cells);
 * row_begin > row_end or row_end > the row count; a query index >= the row
 * count, naming rows[i]; a value outside its feature's domain, naming row and
 * feature; a resident label without a slot (an engine bug), naming engine and
 * row.  The last three are found on the device and ride on the call's one
 * download: one host wait per call.  Scratch: the planes of a chunk of
 * queries and the candidates, 8 k bytes per (query, slice of the targets),
 * each under 1 GiB; "debug.predict_chunk" of the first engine bounds a slice's
 * rows and a chunk's queries.  The engines are read as dist_gibbs_assignments
 * reads them; nothing in them changes.
 * _dev: value columns, row indices and outputs are device pointers.
 * dist_gibbs_search_resident and dist_gibbs_coassign_resident_topk: m == 1. */
int dist_gibbs_search_resident_many_dev(
    dist_gibbs_t * const * engines, size_t m, size_t n_q,
    const uint32_t * const * values_dev, size_t row_begin, size_t row_end,
    size_t k, unsigned flags, uint32_t * index_out_dev, float * prob_out_dev,
    size_t ld);
int dist_gibbs_search_resident_many(
    dist_gibbs_t * const * engines, size_t m, size_t n_q,
    const uint32_t * const * values, size_t row_begin, size_t row_end,
    size_t k, unsigned flags, uint32_t * index_out, float * prob_out,
    size_t ld);
int dist_gibbs_search_resident_dev(
    dist_gibbs_t * g, size_t n_q, const uint32_t * const * values_dev,
    size_t row_begin, size_t row_end, size_t k, unsigned flags,
    uint32_t * index_out_dev, float * prob_out_dev, size_t ld);
int dist_gibbs_search_resident(
    dist_gibbs_t * g, size_t n_q, const uint32_t * const * values,
    size_t row_begin, size_t row_end, size_t k, unsigned flags,
    uint32_t * index_out, float * prob_out, size_t ld);
int dist_gibbs_coassign_resident_topk_many_dev(
    dist_gibbs_t * const * engines, size_t m, const uint32_t * rows_dev,
    size_t n_q, size_t row_begin, size_t row_end, size_t k, unsigned flags,
    uint32_t * index_out_dev, float * prob_out_dev, size_t ld);
int dist_gibbs_coassign_resident_topk_many(
    dist_gibbs_t * const * engines, size_t m, const uint32_t * rows,
    size_t n_q, size_t row_begin, size_t row_end, size_t k, unsigned flags,
    uint32_t * index_out, float * prob_out, size_t ld);
int dist_gibbs_coassign_resident_topk_dev(
    dist_gibbs_t * g, const uint32_t * rows_dev, size_t n_q, size_t row_begin,
    size_t row_end, size_t k, unsigned flags, uint32_t * index_out_dev,
    float * prob_out_dev, size_t ld);
int dist_gibbs_coassign_resident_topk(
    dist_gibbs_t * g, const uint32_t * rows, size_t n_q, size_t row_begin,
    size_t row_end, size_t k, unsigned flags, uint32_t * index_out,
    float * prob_out, size_t ld);

size_t dist_gibbs_group_count(const dist_gibbs_t * g);     /* counts().size() */
size_t dist_gibbs_row_count(const dist_gibbs_t * g);
int dist_gibbs_counts(const dist_gibbs_t * g, int * out);  /* driver counts() */
int dist_gibbs_assignments(const dist_gibbs_t * g, uint32_t * global_out);
int dist_gibbs_get_group(const dist_gibbs_t * g, int feature, size_t groupid,
                         uint32_t * group_out);
int dist_gibbs_packed_to_global(const dist_gibbs_t * g, uint32_t packed,
                                uint32_t * global_out);
int dist_gibbs_global_to_packed(const dist_gibbs_t * g, uint32_t global,
                                uint32_t * packed_out);
/* MixtureIdTracker::global_size (mixture.hpp:517): ids handed out so far */
size_t dist_gibbs_global_size(const dist_gibbs_t * g);
/* Mixture::validate for the whole engine (mixture.hpp:152-163 the driver's
 * _validate, :440-444 the slaves'), as far as the rows themselves can vouch:
 * every row's group id is live; group sizes, and every integer statistic of
 * every feature (count_sum and cells, heads/tails, count/sum; the count of a
 * NormalInverseChiSq group), equal a recount from the rows on the device; the
 * host's mirror of the group set (sizes, empty groups, id maps) equals the
 * device's; there is an empty group; sizes sum to the rows assigned.  Closes
 * an open device-normalised run first; fails while a batch is open.
 * Returns 0 when consistent; 2 with dist_last_error() and *report (may be
 * NULL) naming the first inconsistency; 1 when the check itself failed.
 * Cost: one pass of atomics over the rows + O(K * dim); a diagnostic. */
typedef struct dist_validate_report {
    int code;            /* 0 ok | 1 dead id (group = row, detail = id) |
                            2 value out of range (group = row) | 3 group size |
                            4 statistic 0 | 5 statistic 1 | 6 count cell
                            (detail = value) | 7 host mirror               */
    int feature;         /* -1: the driver                                  */
    long long group;     /* packed group index (or the row, codes 1-2)      */
    long long detail;
    long long expected;  /* the recount                                     */
    long long found;     /* the live statistic                              */
    long long rows_assigned;
    char what[96];
} dist_validate_report_t;
int dist_gibbs_validate(dist_gibbs_t * g, dist_validate_report_t * report);

/* whether THIS rank could run a sharded pass of n_batches batches of
 * batch_rows rows with the group set normalised on the device (a diagnostic:
 * dist_gibbs_sweep_sharded asks every rank itself and takes the device path
 * only when all of them can; "sharded_device_normalise", default 1, set to 0
 * on a rank keeps all of them on the host-normalised loop) */
int dist_gibbs_sharded_device_normalise_ok(const dist_gibbs_t * g,
                                           size_t n_batches,
                                           size_t batch_rows, int * ok_out);
/* Options.  Ten are public; each names the test that exercises it.  None but
 * the last two changes a result.
 *
 *  "value_sorted"  0 generic kernels only | 1 auto (default) | 2 the
 *      value-sorted kernels whenever the feature list allows (ONE feature with
 *      a small value domain).  tests/test_gpu_sweep.py::test_batch_sweeps_bit_exact
 *  "value_stream"  0 per-value tables always | 1 auto (default: the table-free
 *      kernel k_vs_stream where a value has about one tile per batch -- C5) |
 *      2 always.  test_gpu_sweep.py::test_stream_kernel_on_full_tiles,
 *      test_gpu_fullsize.py::test_c5_stream_kernel_where_the_bench_runs_it
 *  "narrow_tiles"  0 never | 1 auto (default: launches too small to fill the
 *      chip take tiles of 64 rows, vectors from LDS: k_vs_narrow) | 2 whenever
 *      the vectors fit.  test_gpu_sweep.py::test_batch_sweeps_bit_exact (modes 4, 5)
 *  "device_normalise"  1 | 2 (default; the same as 1) sweeps that stay on the
 *      value-sorted path with integer statistics normalise the group set on
 *      the device, no host round trip per batch; such a run stays OPEN when
 *      dist_gibbs_sweep / dist_gibbs_sweep_sharded return (the next sweep of
 *      the same tiling goes on with it, any other call pulls the host's
 *      mirrors first), so they return before the device has finished.  An
 *      open run is queued on the stream of the thread that swept; a call from
 *      another thread drains that stream before it reads the state.  0 never.
 *      test_gpu_sweep.py::test_device_side_normalisation_under_group_churn
 *  "sharded_device_normalise"  1 (default) lets dist_gibbs_sweep_sharded do the
 *      same: when a run is opened the ranks agree among themselves (one
 *      all-reduce of a flag) whether every one of them can; 0 keeps this
 *      rank, and so all of them, on the host-normalised loop.  Whether an
 *      open run GOES ON needs no word between them: it follows from the
 *      call's tiling and the batches the run has left, the same on every
 *      rank, and a rank that closed its run between two passes (any look at
 *      its state does) takes it up again with the same bound on the group
 *      count and the same batches left -- the collectives its peers issue.
 *      So READ-ONLY calls between two passes need not be the same on every
 *      rank; calls that change the state must be, as for any replicated state.
 *      tests/test_gpu_native_comm.py (a peek between passes: resumed_runs)
 *  "fused_tables"  1 (default) a device-normalised run spends ONE launch between
 *      a batch's statistics and the next batch's sampling (k_vs_tables: group
 *      set, caches, per-value tables) and the rows a tile hands over are
 *      sampled by k_vs_apply | 0 k_normalise, k_batch_finish, k_vs_prepare and
 *      k_rows_wave as launches of their own -- the path every batch takes
 *      that is NOT part of a device-normalised run of integer statistics
 *      (float statistics: GammaPoisson, NormalInverseChiSq; LowEntropy; more
 *      than 8128 groups; apply chunks of several values; the table-free
 *      kernel).  test_device_side_normalisation_under_group_churn,
 *      test_fused_batches_with_values_of_several_apply_chunks
 *  "kernel_timing"  n: HIP events around the score+sample kernel of every n-th
 *      batch feed dist_gibbs_kernel_stats (1, the default: every batch; 0
 *      none; two events cost a batch some 8 us).
 *      test_gpu_sweep.py::test_kernel_timing_samples_every_nth_batch
 *  "phase_timing"  1: events at a sub-sweep's phase boundaries feed
 *      dist_gibbs_phase_stats (bench.py's step_breakdown); default 0.
 *      tests/test_bench_cli.py
 *  "float_stats"  0 (default) float statistics by the ordered replay | 1 merged
 *      sums (dist_gibbs_float_delta_words): TOLERANCE-LEVEL.
 *      tests/test_gpu_scan.py, tests/test_gpu_fullsize_modes.py
 *  "sampling"  0 (default, the line of record: the reference's float
 *      operations in the reference's order, bit-identical assignments) | 1 SCAN
 *      SAMPLING, TOLERANCE-LEVEL: the same scores bit for bit and the same
 *      engine step per row, but the softmax and its inverse CDF by a running
 *      log-sum-exp and cumulative sums (random.hpp:316-333 in distribution;
 *      the index can differ where u * total falls within float rounding of a
 *      boundary between two groups).  tests/test_gpu_scan.py,
 *      tests/test_gpu_fullsize_modes.py
 *
 * Test hooks, spelled "debug.<name>": each forces a kernel variant the library
 * otherwise picks by itself, so that the differential fuzz (tools/fuzz.py,
 * tests/test_gpu_fuzz.py) reaches every variant at every size; not for
 * callers, and none changes a result.  (The library's table of options,
 * kGibbsOptions in dist_hip.hip, has a row per name listed here;
 * tests/test_gpu_launch_lds.py holds the two lists together.)
 *
 *  "debug.sequential_chain"  2 (default) the exact chain with its structural
 *      steps on the device (k_chains) | 1 the chain kernel that returns to the
 *      host at every structural step | 0 rows as batches of one
 *  "debug.running_sums_min_tiles"  n >= 0: launches of at least this many
 *      tiles use the per-value running sums and band tiles (2048)
 *  "debug.narrow_read_ahead"  k_vs_narrow's instance: 0 by launch size
 *      (default) | 4 | 8 float4s
 *  "debug.stream_scratch"  k_vs_stream keeps a tile's likelihoods between its
 *      passes: 1 (default) | 0 computes them again
 *  "debug.rows_scratch"  general rows: 3 k_rows_scratch (default) | 0
 *      k_sweep_program, which feature lists beyond 64 parameter slots take
 *      anyway
 *  "debug.rows_scratch_lds_log"  FastLog's table in LDS: 1 (default) | 0
 *  "debug.rows_scratch_block"  threads per workgroup of that kernel: a
 *      multiple of 64 up to 1024 (512)
 *  "debug.rows_fold"  leading discrete features folded into a per-(joint
 *      value, group) table: 1 where 128 rows share a value (default) | 2
 *      whenever the joint domain fits | 0
 *  "debug.apply_stage"  general rows' integer statistics summed in LDS: 1
 *      (default) | 0
 *  "debug.program_all"  every batch outside the value-sorted path through the
 *      per-batch score program: 1 (default) | 0
 *  "debug.sample_prio"  wave priorities by phase in k_vs_sample and
 *      k_vs_stream: 0x13210 (default: set-up, first pass, ..., last pass) | 0
 *      none | 0x1abcd -- the A/B of profiles/r5_wave_priorities.txt
 *  "debug.rows_prio"  the same in k_rows_scratch
 *  "debug.apply_overlap"  k_vs_apply samples a chunk's few handed-over rows
 *      while its other waves add up the moves: 1 (default) | 0 before they do
 *  "debug.run_batches_cap"  n >= 0: a device-normalised run covers at most
 *      this many batches, 0 (default) as many as fit --
 *      tests/test_gpu_native_ranks.py sees a run used up and the ranks agree
 *      on the next one
 *  "debug.shared_totals"  k_vs_tables folds every (value, group) cell's
 *      sampling total and the tiles skip their total pass: 0 never | 1 where
 *      the library chooses (default) | 2 whenever k_vs_tables runs.
 *      tests/test_gpu_shared_totals.py
 *  "debug.score_rows_chunk"  n > 0: the most (row, group) work-items one
 *      dist_gibbs_score_rows_dev launch takes (2^30)
 *  "debug.predict_chunk"  n > 0: the most query rows one dist_gibbs_predict
 *      or dist_gibbs_predict_feature launch takes (2^22)
 */
int dist_gibbs_set_option(dist_gibbs_t * g, const char * name, int value);
/* The certified search.  EXACT at every setting.  k_vs_search, in
 * k_vs_sample's place, answers a row's inverse CDF by binary search on the
 * value's float64 prefix sums where a bound on the float chain's rounding
 * proves the index (csrc/vs_certify.h), and runs the chain itself on the rows
 * that are left over.  mode: 0 never | 1 where the library chooses (default)
 * | 2 wherever it applies (a fused batch with shared totals whose search
 * tables fit the LDS).  slack in 0..200, for tests: the bound times 2^slack
 * (default 0), so that small shapes leave rows to the chain; 200 certifies
 * nothing.  tests/test_gpu_certified_search.py */
int dist_gibbs_set_certified_search(dist_gibbs_t * g, int mode, int slack);
/* how many batches each score+sample kernel has served */
int dist_gibbs_path_counts(const dist_gibbs_t * g, uint64_t * value_sorted,
                           uint64_t * generic);
/* diagnostics for the tests: out[0..20] = batches through the value-sorted
 * kernel, through the other kernels, launches with band tiles on, launches
 * with running sums on, values whose arg-max rows had their own tile in the
 * last value-sorted launch, rows that launch handed to the wave-per-row
 * kernel, value-sorted batches that took the table-free kernel, batches
 * whose group set the device normalised itself, value-sorted batches that
 * took the small-launch kernel, batches through k_rows_scratch, batches with
 * folded leading features, batches sampled in scan mode, batches with merged
 * float statistics, batches whose group set, caches and tables came from the
 * one fused launch, sharded runs this rank closed between two passes and took
 * up again, launches of the exact-chain kernel k_chains this engine issued,
 * out[16] the leading ops the last k_rows_scratch launch folded into its
 * per-(joint value, group) table, out[17] the instance that launch took by
 * the ops that remained (0 generic, 1 GN, 2 N, 3 NN, 4 G, 5 C; G a table
 * gather, C a categorical, N a NormalInverseChiSq); both 0 before any such
 * launch; out[18] batches that took the certified search, out[19] the rows
 * it answered itself and out[20] the rows it left to the chain, summed over
 * those batches (first min(n, 21) entries are written) */
int dist_gibbs_debug_counts(dist_gibbs_t * g, uint64_t * out, size_t n);
/* "phase_timing" = 1 (a diagnostic: six events per sub-sweep): HIP-event time
 * (ms, summed) of the five phases of the device-normalised value-sorted
 * sub-sweeps since the last reset -- the per-value tables, the score+sample
 * kernel, the handed-over rows, the statistics, the group set and caches --
 * and how many sub-sweeps were timed */
int dist_gibbs_phase_stats(dist_gibbs_t * g, double ms_out[5],
                           uint64_t * batches_out, int reset);
/* HIP-event time (ms) and count of the all-reduces dist_gibbs_sweep_sharded
 * timed (every "kernel_timing"-th sub-sweep) since the last reset */
int dist_gibbs_comm_stats(dist_gibbs_t * g, double * ms_out,
                          uint64_t * launches_out, int reset);
/* HIP-event time (ms) and launch count of the score+sample kernel since the
 * last reset, measured on the engine's stream */
int dist_gibbs_kernel_stats(dist_gibbs_t * g, double * ms_out,
                            uint64_t * launches_out, uint64_t * rows_out,
                            int reset);

/* ---- engine hyper-parameters -------------------------------------------
 * The reference's mixture interface alternates assignment sweeps
 * (mixture.hpp:73-122) with a hyper-parameter step: score a grid of candidate
 * Shareds against the groups (MixtureSlave::score_data_grid), draw one
 * (sample_from_scores), install it and init().  These entry points are that
 * step on the statistics the engine holds: nothing is pulled to the host, no
 * second mixture is built, the rows and id maps stay where they are.
 *
 * Two rules hold for all of them:
 *  - dist_gibbs_shared, dist_gibbs_clustering, dist_gibbs_score_data,
 *    dist_gibbs_score_data_grid and dist_gibbs_score_counts_grid are READERS.
 *    They close an open device-normalised run but leave a sharded run this
 *    rank closed resumable.  The scoring ones read every cell of the feature:
 *    on a value-partitioned rank whose cells are stale they fail ("... are
 *    stale on a value-partitioned rank") until dist_gibbs_gather_cells.
 *  - dist_gibbs_set_* and dist_gibbs_sample_* are NOT readers: they close the
 *    run and forget it.  On sharded engines every rank issues them alike;
 *    replicas that call dist_gibbs_sample_* with equal rng_state choose the
 *    same index, because their statistics are equal (DirichletProcessDiscrete
 *    excepted: its binary64 sums are formed by atomics, see below).
 * All of them fail while a batch is open (between dist_gibbs_batch_sample and
 * dist_gibbs_batch_finish). */

/* Model::Shared of one feature as the engine currently runs under it (the
 * constructor argument, or what dist_gibbs_set_shared / dist_gibbs_sample_
 * hypers installed since).  DirichletProcessDiscrete: out->betas must point at
 * dim floats owned by the caller, which are written. */
int dist_gibbs_shared(const dist_gibbs_t * g, int feature,
                      dist_shared_t * out);
/* PitmanYor's (alpha, d); fails on a LowEntropy engine */
int dist_gibbs_clustering(const dist_gibbs_t * g, float * alpha, float * d);
/* MixtureSlave::score_data (mixture.hpp:427-431) of every feature --
 * per_feature[n_features] -- and score_counts of the engine's clustering
 * model over its group sizes: PitmanYor::score_counts (clustering.cc:152-183),
 * or LowEntropy::score_counts (clustering.cc:229-248) for an engine of
 * dist_gibbs_create_low_entropy */
int dist_gibbs_score_data(dist_gibbs_t * g, float * per_feature,
                          float * clustering);
/* MixtureSlave::score_data_grid (mixture.hpp:433-438, 238-247; dd.hpp:259-284)
 * on the resident statistics: scores_out[c] = score_data under shareds[c].
 * Kind and dim of every candidate are the feature's.  The float contract is
 * dist_mixture_score_data_grid's: DirichletDiscrete and the scalar kinds in
 * the reference's float accumulation order, bit for bit (DirichletDiscrete's
 * alpha_sum carried in binary64 from candidate to candidate over the changed
 * coordinates); DirichletProcessDiscrete in binary64, 1e-5 relative.
 * DirichletDiscrete's work follows what changed: one accumulator chain per
 * distinct (coordinate, alpha) and per distinct alpha_sum of the grid, so a
 * coordinate grid of n candidates costs dim + 1 + 2 (n - 1) chains, not
 * n (dim + 1). */
int dist_gibbs_score_data_grid(dist_gibbs_t * g, int feature,
                               const dist_shared_t * shareds, size_t n,
                               float * scores_out);
/* PitmanYor::score_counts (clustering.cc:152-183) of the engine's group sizes
 * under every (alphas[c], ds[c]).  Fails on a LowEntropy engine, whose model
 * has no such parameters. */
int dist_gibbs_score_counts_grid(dist_gibbs_t * g, const float * alphas,
                                 const float * ds, size_t n,
                                 float * scores_out);
/* Shared = candidate; init() (mixture.hpp:354-359).  The candidate is checked
 * first (kind and dim unchanged, and what dist_gibbs_create checks); a refused
 * candidate leaves the engine as it was.  Then everything derived from the
 * hyper-parameters is rebuilt: the feature's prior tables and registered small
 * lgamma arguments, the caches over the groups, and with them what the next
 * batch or chain builds (per-value tables, base scores).  From then on the
 * engine is indistinguishable from one created with the new values and handed
 * the same groups, sizes and id maps; the sufficient statistics -- the
 * order-dependent ones included -- do not depend on the hyper-parameters and
 * stay as they are. */
int dist_gibbs_set_shared(dist_gibbs_t * g, int feature,
                          const dist_shared_t * shared);
/* the same for PitmanYor's (alpha, d) (clustering.hpp:151-161); fails on a
 * LowEntropy engine */
int dist_gibbs_set_clustering(dist_gibbs_t * g, float alpha, float d);
/* The whole step: the grid as in dist_gibbs_score_data_grid, then
 * sample_from_scores_overwrite (random.hpp:361-392) on the device with ONE
 * engine step from *rng_state, then dist_gibbs_set_shared of the chosen
 * candidate.  Only *chosen and the advanced *rng_state cross the bus; the
 * scores never do.  n > 0. */
int dist_gibbs_sample_hypers(dist_gibbs_t * g, int feature,
                             const dist_shared_t * shareds, size_t n,
                             uint32_t * rng_state, size_t * chosen);
/* ... and for the clustering model: dist_gibbs_score_counts_grid, the draw,
 * dist_gibbs_set_clustering */
int dist_gibbs_sample_clustering(dist_gibbs_t * g, const float * alphas,
                                 const float * ds, size_t n,
                                 uint32_t * rng_state, size_t * chosen);
/* A whole coordinate pass of a DirichletDiscrete feature in one call: for
 * every step i, a grid of grid_size values for alphas[coords[i]] is scored
 * (MixtureSlave::score_data_grid, mixture.hpp:433-438, in DirichletDiscrete's
 * incremental form, dd.hpp:259-284), one is drawn (sample_from_scores_
 * overwrite, random.hpp:361-392) and takes the coordinate's place.  It is
 * DEFINED as this loop of dist_gibbs_sample_hypers calls and gives its result
 * bit for bit -- chosen[], the advanced *rng_state, the Shared in force
 * afterwards and everything derived from it:
 *
 *     alphas = the feature's alphas in force
 *     for i in 0 .. n_coords-1:
 *         v = coords[i];  row = grid + i * grid_stride
 *         candidate c = alphas with alphas[v] = row[c],  c < grid_size
 *         dist_gibbs_sample_hypers(g, feature, candidates, grid_size,
 *                                  rng_state, &chosen[i])
 *         alphas[v] = row[chosen[i]]
 *
 * coords may be in any order and may repeat (a coordinate visited again sees
 * its earlier draw); grid_stride == 0 gives every step the same grid_size
 * values, otherwise grid_stride >= grid_size floats lie between the steps'
 * rows.  Each step takes one engine step of *rng_state; n_coords == 0 changes
 * nothing and leaves the state as given.  The loop's bit rules: candidate 0's
 * alpha_sum is the float sum of its alphas in index order, the following ones
 * carry it in binary64 over the changed coordinate (only where the floats
 * differ) and narrow it; a coordinate's accumulator is the float sum over the
 * groups with members, in index order, of fast_lgamma(a + count) -
 * fast_lgamma(a), the shift accumulator that of fast_lgamma(alpha_sum) -
 * fast_lgamma(alpha_sum + size); a score is vector_sum over the dim + 1
 * accumulators in the association the reference was built with.
 *
 * NOT readers, like dist_gibbs_sample_hypers: they fail while a batch is open
 * and on a value-partitioned rank with stale cells, and forget a run.
 * Everything is checked before anything is launched or installed -- the
 * feature index; its kind (DirichletDiscrete, otherwise the call fails naming
 * the kind); coords[i] in [0, dim); 1 <= grid_size <= INT_MAX; every grid value
 * finite and > 0, which a DirichletDiscrete alpha has to be; _many: engines
 * non-null and distinct, at most 65535, the feature of one dim across them --
 * and a refused call leaves every engine as it was.
 *
 * The device runs the pass in 2 launches whatever n_coords, grid_size and m
 * are: every accumulator chain of the pass at once (one per coordinate under
 * the alphas in force and one per distinct (coords[i], grid value), the
 * latter shared by all engines), then one workgroup per engine that walks the
 * steps -- alpha_sums, shift accumulators, closing sums, draw -- and leaves
 * chosen[] and the state for the host's single wait; the final alphas are
 * installed once per engine as dist_gibbs_set_shared does.  Where the loop's
 * arithmetic cannot be reproduced without the host, the engine concerned runs
 * the loop itself, whose result is the same by definition:
 *  - an alpha_sum below 2.5 is reachable: fast_lgamma then takes glibc's
 *    lgammaf per registered argument, and which sums occur depends on the
 *    draws.  Decided from the binary64 sum, over the coordinates, of the
 *    smallest value each can hold (its alpha in force, its grid values if a
 *    step visits it): below 3.0 the loop runs.  A float sum of dim <= 256
 *    positive terms lies within 256 * 2^-24 < 2e-5 relative of the exact one,
 *    so from 3.0 up no float sum falls below 2.99.  Likewise, by the largest
 *    values, above 1e9: alpha_sum plus a group size must stay clear of
 *    fast_lgamma's 2^32 branch;
 *  - the grid's arguments below 2.5 (value + 0, 1, 2 per distinct value, held
 *    for the call) do not all fit the process-wide table of 16384 at once;
 *    the loop holds one step's at a time;
 *  - no group has a member (no groups at all included): every score is +0;
 *    widened from "no groups" because it costs nothing to tell and the
 *    kernels would have nothing to sum;
 *  - grid_size > 1024 (one lane of the 1024-thread workgroup closes each
 *    candidate) or n_coords * grid_size > 2^24.
 * dist_gibbs_hyper_stats tells which ran: a device pass adds 1 call,
 * n_coords * grid_size candidates, dim + the distinct grid chains + n_coords *
 * grid_size shift chains, and 2 launches, on every engine it served; the loop
 * adds what its dist_gibbs_sample_hypers calls add, 1 call and 3 launches per
 * step.  On sharded engines every rank calls it alike; the chains are summed
 * in a fixed order, so replicas with equal rng_state choose alike. */
int dist_gibbs_sample_hypers_pass(dist_gibbs_t * g, int feature,
        const int * coords, size_t n_coords,
        const float * grid, size_t grid_size,
        size_t grid_stride, /* 0: one grid for every step */
        uint32_t * rng_state, uint32_t * chosen /* [n_coords] */);
/* ... of m engines in the same 2 launches, engine j with rng_states[j], into
 * chosen[j * n_coords + i]; engines that need the loop run it one by one. */
int dist_gibbs_sample_hypers_pass_many(dist_gibbs_t * const * engines, size_t m,
        int feature, const int * coords, size_t n_coords,
        const float * grid, size_t grid_size, size_t grid_stride,
        uint32_t * rng_states /* [m] */, uint32_t * chosen /* [m][n_coords] */);
/* since creation: out[0] = accumulator chains run by DirichletDiscrete grids,
 * out[1] = candidates scored, out[2] = kernel launches of this section,
 * out[3] = calls of its scoring, set and sample entry points (does not close
 * a run) */
int dist_gibbs_hyper_stats(dist_gibbs_t * g, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* DISTRIBUTIONS_HIP_H */
