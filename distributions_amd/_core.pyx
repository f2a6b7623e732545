# cython: language_level=3, boundscheck=False, wraparound=False
"""Cython binding of libdistributions_hip's C ABI (include/distributions_hip.h).

This is the one extension module of the package; the modules under
distributions_amd/lp re-export its classes under the names of the reference's
distributions.lp wrappers (distributions/lp/models/_dd.pyx etc.).  It does no
arithmetic of its own: every score, cache entry and sample comes from the HIP
library.  Errors of the library surface as RuntimeError, like the reference's
`except +` translation of std::runtime_error.
"""
from libc.stdint cimport uint8_t, uint32_t, uint64_t, int32_t
from libc.stddef cimport size_t
from libc.string cimport memset, memcpy
from libc.stdlib cimport malloc, free

import numpy as np
cimport numpy as cnp

cnp.import_array()

cdef extern from "distributions_hip.h" nogil:
    enum:
        DIST_DD
        DIST_BB
        DIST_GP
        DIST_NICH
        DIST_DPD
        DIST_BNB
    ctypedef struct dist_shared_t:
        int kind
        int dim
        float p[4]
        float alphas[256]
        const float * betas
    size_t dist_group_words(const dist_shared_t *)
    int dist_abi_version()
    const char * dist_last_error()
    int dist_device_count(int *)
    int dist_set_device(int)
    int dist_synchronize()
    int dist_set_stream(void *)
    uint32_t dist_rng_seed(uint64_t)
    uint32_t dist_rng_next(uint32_t *)
    float dist_rng_unif01(uint32_t *)
    uint32_t dist_rng_jump(uint32_t, uint64_t)
    int dist_vector_log(size_t, const float *, float *)
    int dist_vector_exp(size_t, const float *, float *)
    int dist_vector_lgamma(size_t, const float *, float *)
    int dist_vector_lgamma_nu(size_t, const float *, float *)
    int dist_vector_log_factorial(size_t, const uint32_t *, float *)
    int dist_sample_from_scores_overwrite(uint32_t *, size_t, float *, size_t *)
    int dist_scores_to_likelihoods(size_t, float *, float *)
    int dist_sample_from_likelihoods(uint32_t *, size_t, const float *, float,
                                     size_t *)
    int dist_log_sum_exp(size_t, const float *, float *)
    int dist_py_score_add_value(float, float, int, int, int, int, float *)
    int dist_py_score_remove_value(float, float, int, int, int, int, float *)
    int dist_py_score_counts(float, float, const int *, size_t, float *)
    int dist_py_sample_assignments(float, float, int, uint32_t *, int *)

    ctypedef struct dist_py_mixture_t:
        pass
    ctypedef struct dist_le_mixture_t:
        pass
    int dist_le_score_add_value(int, int, int, int, int, float *)
    int dist_le_score_remove_value(int, int, int, int, int, float *)
    int dist_le_log_partition_function(int, float *)
    int dist_le_sample_assignments(int, int, uint32_t *, int *)
    int dist_le_score_counts(int, const int *, size_t, float *)
    dist_le_mixture_t * dist_le_mixture_create()
    void dist_le_mixture_destroy(dist_le_mixture_t *)
    int dist_le_mixture_init(dist_le_mixture_t *, const int *, size_t)
    int dist_le_mixture_add_value(dist_le_mixture_t *, size_t, int *)
    int dist_le_mixture_remove_value(dist_le_mixture_t *, size_t, int *)
    int dist_le_mixture_score_value(const dist_le_mixture_t *, int, float *,
                                    size_t)
    int dist_le_mixture_score_data(const dist_le_mixture_t *, int, float *)
    size_t dist_le_mixture_size(const dist_le_mixture_t *)
    size_t dist_le_mixture_sample_size(const dist_le_mixture_t *)
    int dist_le_mixture_counts(const dist_le_mixture_t *, int *)
    dist_py_mixture_t * dist_py_mixture_create()
    void dist_py_mixture_destroy(dist_py_mixture_t *)
    int dist_py_mixture_init(dist_py_mixture_t *, float, float, const int *,
                             size_t)
    int dist_py_mixture_add_value(dist_py_mixture_t *, float, float, size_t,
                                  int *)
    int dist_py_mixture_remove_value(dist_py_mixture_t *, float, float, size_t,
                                     int *)
    int dist_py_mixture_score_value(const dist_py_mixture_t *, float, float,
                                    float *, size_t)
    int dist_py_mixture_score_data(const dist_py_mixture_t *, float, float,
                                   float *)
    size_t dist_py_mixture_size(const dist_py_mixture_t *)
    size_t dist_py_mixture_sample_size(const dist_py_mixture_t *)
    int dist_py_mixture_counts(const dist_py_mixture_t *, int *)
    size_t dist_py_mixture_empty_groupids(const dist_py_mixture_t *, size_t *,
                                          size_t)

    ctypedef struct dist_mixture_t:
        pass
    dist_mixture_t * dist_mixture_create(const dist_shared_t *)
    void dist_mixture_destroy(dist_mixture_t *)
    int dist_mixture_clear(dist_mixture_t *)
    int dist_mixture_append(dist_mixture_t *, const uint32_t *)
    int dist_mixture_get_group(const dist_mixture_t *, size_t, uint32_t *)
    size_t dist_mixture_size(const dist_mixture_t *)
    int dist_mixture_init(dist_mixture_t *)
    int dist_mixture_add_group(dist_mixture_t *)
    int dist_mixture_remove_group(dist_mixture_t *, size_t)
    int dist_mixture_add_value(dist_mixture_t *, size_t, uint32_t)
    int dist_mixture_remove_value(dist_mixture_t *, size_t, uint32_t)
    int dist_mixture_score_value_group(const dist_mixture_t *, size_t,
                                       uint32_t, float *)
    int dist_mixture_score_value(const dist_mixture_t *, uint32_t, float *,
                                 size_t)
    int dist_mixture_score_data(const dist_mixture_t *, float *)
    int dist_mixture_validate(const dist_mixture_t *)
    int dist_mixture_score_values(const dist_mixture_t *, const uint32_t *,
                                  size_t, float *, size_t)
    int dist_mixture_score_data_grid(const dist_mixture_t *,
                                     const dist_shared_t *, size_t, float *)

    int dist_group_init(const dist_shared_t *, uint32_t *)
    int dist_group_add_value(const dist_shared_t *, uint32_t *, uint32_t)
    int dist_group_remove_value(const dist_shared_t *, uint32_t *, uint32_t)
    int dist_group_sample_value(const dist_shared_t *, const uint32_t *,
                                uint32_t, uint64_t, size_t, int, uint32_t *)
    int dist_group_score_value(const dist_shared_t *, const uint32_t *,
                               uint32_t, float *)
    int dist_group_score_data(const dist_shared_t *, const uint32_t *, float *)
    ctypedef struct dist_dpd_shared_t:
        pass
    dist_dpd_shared_t * dist_dpd_shared_create()
    void dist_dpd_shared_destroy(dist_dpd_shared_t *)
    int dist_dpd_shared_load(dist_dpd_shared_t *, float, float,
                             const uint32_t *, const float *, const int *,
                             size_t)
    int dist_dpd_shared_add_value(dist_dpd_shared_t *, uint32_t, uint32_t *)
    int dist_dpd_shared_remove_value(dist_dpd_shared_t *, uint32_t)
    int dist_dpd_shared_realize(dist_dpd_shared_t *, uint32_t *)
    size_t dist_dpd_shared_slots(const dist_dpd_shared_t *)
    size_t dist_dpd_shared_size(const dist_dpd_shared_t *)
    uint64_t dist_dpd_shared_version(const dist_dpd_shared_t *)
    int dist_dpd_shared_params(const dist_dpd_shared_t *, float *, float *,
                               float *)
    int dist_dpd_shared_view(const dist_dpd_shared_t *, dist_shared_t *)
    int dist_dpd_shared_slot(const dist_dpd_shared_t *, uint32_t, uint32_t *)
    int dist_dpd_shared_dump(const dist_dpd_shared_t *, uint32_t *, float *,
                             int *)
    int dist_sample_gamma(uint32_t *, float, float, float *)
    int dist_sample_beta_safe(uint32_t *, float, float, float, float *)
    size_t dist_scorer_words(const dist_shared_t *)
    int dist_scorer_init(const dist_shared_t *, const uint32_t *, float *)
    int dist_scorer_eval(const dist_shared_t *, const float *, uint32_t,
                         float *)
    int dist_group_protobuf_dump(const dist_shared_t *, const uint32_t *,
                                 const uint32_t *, uint8_t *, size_t, size_t *)
    int dist_group_protobuf_load(const dist_shared_t *, const uint32_t *,
                                 const uint8_t *, size_t, uint32_t *)
    int dist_shared_protobuf_dump(const dist_shared_t *, uint8_t *, size_t,
                                  size_t *)
    int dist_shared_protobuf_load(int, const uint8_t *, size_t,
                                  dist_shared_t *)

    ctypedef struct dist_id_tracker_t:
        pass
    dist_id_tracker_t * dist_id_tracker_create()
    void dist_id_tracker_destroy(dist_id_tracker_t *)
    int dist_id_tracker_init(dist_id_tracker_t *, size_t)
    int dist_id_tracker_add_group(dist_id_tracker_t *)
    int dist_id_tracker_remove_group(dist_id_tracker_t *, uint32_t)
    int dist_id_tracker_packed_to_global(const dist_id_tracker_t *, uint32_t,
                                         uint32_t *)
    int dist_id_tracker_global_to_packed(const dist_id_tracker_t *, uint32_t,
                                         uint32_t *)
    size_t dist_id_tracker_packed_size(const dist_id_tracker_t *)
    size_t dist_id_tracker_global_size(const dist_id_tracker_t *)

    ctypedef struct dist_gibbs_t:
        pass
    dist_gibbs_t * dist_gibbs_create(float, float, int, const dist_shared_t *)
    dist_gibbs_t * dist_gibbs_create_low_entropy(int, int,
                                                 const dist_shared_t *)
    ctypedef struct dist_comm_t:
        pass
    int dist_comm_available()
    int dist_comm_unique_id(uint8_t *)
    int dist_comm_unique_id_host(uint8_t *)
    dist_comm_t * dist_comm_create(const uint8_t *, int, int)
    int dist_comm_size(const dist_comm_t *, int *, int *)
    int dist_comm_all_reduce_dev(dist_comm_t *, void *, size_t, int, int)
    int dist_gibbs_partition_by_value(dist_gibbs_t *, dist_comm_t *)
    int dist_gibbs_gather_cells(dist_gibbs_t *, dist_comm_t *)
    int dist_gibbs_comm_volume(dist_gibbs_t *, uint64_t *, int)
    void dist_comm_destroy(dist_comm_t *)
    int dist_gibbs_sweep_sharded(dist_gibbs_t *, dist_comm_t *, size_t, size_t,
                                 uint32_t, uint64_t)
    void dist_gibbs_destroy(dist_gibbs_t *)
    int dist_gibbs_load_rows(dist_gibbs_t *, size_t, const uint32_t * const *,
                             const uint32_t *, int, int, uint64_t)
    int dist_gibbs_load_rows_dev(dist_gibbs_t *, size_t,
                                 const uint32_t * const *, uint32_t *, int,
                                 int, uint64_t)
    int dist_gibbs_load_rows_unassigned(dist_gibbs_t *, size_t,
                                        const uint32_t * const *, int,
                                        uint64_t)
    int dist_gibbs_init_sequential(dist_gibbs_t *, size_t, size_t,
                                   uint32_t *, int) nogil
    size_t dist_gibbs_stat_words(const dist_gibbs_t *)
    int dist_gibbs_export_stats_dev(const dist_gibbs_t *, int32_t *)
    int dist_gibbs_import_stats_dev(dist_gibbs_t *, const int32_t *)
    int dist_gibbs_sweep(dist_gibbs_t *, size_t, size_t, size_t, uint32_t,
                         uint64_t)
    int dist_gibbs_sweep_sequential(dist_gibbs_t *, size_t, size_t, uint32_t *)
    int dist_gibbs_sweep_sequential_many(dist_gibbs_t * const *, size_t,
                                         size_t, size_t, uint32_t *) nogil
    int dist_gibbs_batch_sample(dist_gibbs_t *, size_t, size_t, uint32_t,
                                uint64_t)
    int dist_gibbs_batch_delta_dev(dist_gibbs_t *, int32_t *)
    int dist_gibbs_batch_apply_delta_dev(dist_gibbs_t *, const int32_t *)
    int dist_gibbs_ordered_features(const dist_gibbs_t *, int *)
    int dist_gibbs_batch_moves_dev(dist_gibbs_t *, uint32_t *, uint32_t *)
    int dist_gibbs_replay_ordered_dev(dist_gibbs_t *, const uint32_t *,
                                      const uint32_t *,
                                      const uint32_t * const *, size_t, int)
    int dist_gibbs_batch_apply_local(dist_gibbs_t *)
    int dist_gibbs_batch_finish(dist_gibbs_t *)
    int dist_gibbs_row_scores(dist_gibbs_t *, size_t, float *, size_t *)
    int dist_gibbs_score_rows_dev(dist_gibbs_t *, size_t, size_t, float *,
                                  size_t)
    int dist_gibbs_predict_dev(dist_gibbs_t *, size_t,
                               const uint32_t * const *, float *, uint32_t *,
                               int, uint32_t, uint64_t, float *)
    int dist_gibbs_predict(dist_gibbs_t *, size_t, const uint32_t * const *,
                           float *, uint32_t *, int, uint32_t, uint64_t,
                           float *)
    int dist_gibbs_predict_many_dev(dist_gibbs_t * const *, size_t, size_t,
                                    const uint32_t * const *, float *,
                                    uint32_t *, uint32_t *, int, uint32_t,
                                    uint32_t, uint64_t, float *, size_t,
                                    float *, unsigned) nogil
    int dist_gibbs_predict_many(dist_gibbs_t * const *, size_t, size_t,
                                const uint32_t * const *, float *,
                                uint32_t *, uint32_t *, int, uint32_t,
                                uint32_t, uint64_t, float *, size_t, float *,
                                unsigned) nogil
    int dist_gibbs_coassign_many_dev(dist_gibbs_t * const *, size_t, size_t,
                                     const uint32_t * const *, size_t,
                                     const uint32_t * const *, float *,
                                     size_t) nogil
    int dist_gibbs_coassign_many(dist_gibbs_t * const *, size_t, size_t,
                                 const uint32_t * const *, size_t,
                                 const uint32_t * const *, float *,
                                 size_t) nogil
    int dist_gibbs_coassign_dev(dist_gibbs_t *, size_t,
                                const uint32_t * const *, size_t,
                                const uint32_t * const *, float *,
                                size_t) nogil
    int dist_gibbs_coassign(dist_gibbs_t *, size_t, const uint32_t * const *,
                            size_t, const uint32_t * const *, float *,
                            size_t) nogil
    int dist_partition_agreement_dev(size_t, size_t, const uint32_t * const *,
                                     const uint32_t *, uint64_t *,
                                     double *) nogil
    int dist_partition_agreement(size_t, size_t, const uint32_t * const *,
                                 const uint32_t *, uint64_t *, double *) nogil
    int dist_gibbs_partition_agreement_many_dev(
        dist_gibbs_t * const *, size_t, size_t, const uint32_t * const *,
        size_t, const uint32_t *, uint64_t *, double *) nogil
    int dist_gibbs_partition_agreement_many(
        dist_gibbs_t * const *, size_t, size_t, const uint32_t * const *,
        size_t, const uint32_t *, uint64_t *, double *) nogil
    int dist_gibbs_partition_agreement(
        dist_gibbs_t *, size_t, const uint32_t * const *, size_t,
        const uint32_t *, uint64_t *, double *) nogil
    int dist_gibbs_coassign_resident_many_dev(
        dist_gibbs_t * const *, size_t, const uint32_t *, size_t,
        const uint32_t *, size_t, float *, size_t) nogil
    int dist_gibbs_coassign_resident_many(
        dist_gibbs_t * const *, size_t, const uint32_t *, size_t,
        const uint32_t *, size_t, float *, size_t) nogil
    int dist_gibbs_coassign_resident_dev(
        dist_gibbs_t *, const uint32_t *, size_t, const uint32_t *, size_t,
        float *, size_t) nogil
    int dist_gibbs_coassign_resident(
        dist_gibbs_t *, const uint32_t *, size_t, const uint32_t *, size_t,
        float *, size_t) nogil
    int dist_gibbs_search_resident_many_dev(
        dist_gibbs_t * const *, size_t, size_t, const uint32_t * const *,
        size_t, size_t, size_t, unsigned, uint32_t *, float *, size_t) nogil
    int dist_gibbs_search_resident_many(
        dist_gibbs_t * const *, size_t, size_t, const uint32_t * const *,
        size_t, size_t, size_t, unsigned, uint32_t *, float *, size_t) nogil
    int dist_gibbs_search_resident_dev(
        dist_gibbs_t *, size_t, const uint32_t * const *, size_t, size_t,
        size_t, unsigned, uint32_t *, float *, size_t) nogil
    int dist_gibbs_search_resident(
        dist_gibbs_t *, size_t, const uint32_t * const *, size_t, size_t,
        size_t, unsigned, uint32_t *, float *, size_t) nogil
    int dist_gibbs_coassign_resident_topk_many_dev(
        dist_gibbs_t * const *, size_t, const uint32_t *, size_t, size_t,
        size_t, size_t, unsigned, uint32_t *, float *, size_t) nogil
    int dist_gibbs_coassign_resident_topk_many(
        dist_gibbs_t * const *, size_t, const uint32_t *, size_t, size_t,
        size_t, size_t, unsigned, uint32_t *, float *, size_t) nogil
    int dist_gibbs_coassign_resident_topk_dev(
        dist_gibbs_t *, const uint32_t *, size_t, size_t, size_t, size_t,
        unsigned, uint32_t *, float *, size_t) nogil
    int dist_gibbs_coassign_resident_topk(
        dist_gibbs_t *, const uint32_t *, size_t, size_t, size_t, size_t,
        unsigned, uint32_t *, float *, size_t) nogil
    int dist_gibbs_coassign_topk_many_dev(
        dist_gibbs_t * const *, size_t, size_t, const uint32_t * const *,
        size_t, const uint32_t * const *, size_t, unsigned, uint32_t *,
        float *, size_t) nogil
    int dist_gibbs_coassign_topk_many(
        dist_gibbs_t * const *, size_t, size_t, const uint32_t * const *,
        size_t, const uint32_t * const *, size_t, unsigned, uint32_t *,
        float *, size_t) nogil
    int dist_gibbs_coassign_topk_dev(
        dist_gibbs_t *, size_t, const uint32_t * const *, size_t,
        const uint32_t * const *, size_t, unsigned, uint32_t *, float *,
        size_t) nogil
    int dist_gibbs_coassign_topk(
        dist_gibbs_t *, size_t, const uint32_t * const *, size_t,
        const uint32_t * const *, size_t, unsigned, uint32_t *, float *,
        size_t) nogil
    int dist_gibbs_responsibilities_dev(dist_gibbs_t *, size_t,
                                        const uint32_t * const *, float *,
                                        size_t) nogil
    int dist_gibbs_responsibilities(dist_gibbs_t *, size_t,
                                    const uint32_t * const *, float *,
                                    size_t) nogil
    int dist_gibbs_predict_feature_dev(dist_gibbs_t *, size_t,
                                       const uint32_t * const *,
                                       const uint32_t *, int,
                                       const uint32_t *, size_t, float *,
                                       float *, uint32_t *, int, uint32_t,
                                       uint64_t, unsigned)
    int dist_gibbs_predict_feature(dist_gibbs_t *, size_t,
                                   const uint32_t * const *,
                                   const uint32_t *, int, const uint32_t *,
                                   size_t, float *, float *, uint32_t *, int,
                                   uint32_t, uint64_t, unsigned)
    int dist_gibbs_predict_feature_many_dev(
        dist_gibbs_t * const *, size_t, size_t, const uint32_t * const *,
        const uint32_t *, int, const uint32_t *, size_t, float *, float *,
        uint32_t *, uint32_t *, int, uint32_t, uint32_t, uint64_t, float *,
        size_t, float *, size_t, float *, unsigned) nogil
    int dist_gibbs_predict_feature_many(
        dist_gibbs_t * const *, size_t, size_t, const uint32_t * const *,
        const uint32_t *, int, const uint32_t *, size_t, float *, float *,
        uint32_t *, uint32_t *, int, uint32_t, uint32_t, uint64_t, float *,
        size_t, float *, size_t, float *, unsigned) nogil
    int dist_gibbs_sample_rows_dev(dist_gibbs_t *, size_t,
                                   const uint32_t * const *,
                                   const uint32_t *, uint32_t * const *,
                                   uint32_t *, uint32_t, uint64_t)
    int dist_gibbs_sample_rows(dist_gibbs_t *, size_t,
                               const uint32_t * const *, const uint32_t *,
                               uint32_t * const *, uint32_t *, uint32_t,
                               uint64_t)
    int dist_gibbs_sample_rows_many_dev(
        dist_gibbs_t * const *, size_t, size_t, const uint32_t * const *,
        const uint32_t *, uint32_t * const *, uint32_t *, uint32_t *, float *,
        uint32_t, uint32_t, uint64_t, unsigned) nogil
    int dist_gibbs_sample_rows_many(
        dist_gibbs_t * const *, size_t, size_t, const uint32_t * const *,
        const uint32_t *, uint32_t * const *, uint32_t *, uint32_t *, float *,
        uint32_t, uint32_t, uint64_t, unsigned) nogil
    int dist_gibbs_marginals_dev(dist_gibbs_t *, size_t,
                                 const uint32_t * const *, const uint32_t *,
                                 size_t, float *) nogil
    int dist_gibbs_marginals(dist_gibbs_t *, size_t, const uint32_t * const *,
                             const uint32_t *, size_t, float *) nogil
    int dist_gibbs_marginals_many_dev(
        dist_gibbs_t * const *, size_t, size_t, const uint32_t * const *,
        const uint32_t *, size_t, float *, float *, size_t, float *) nogil
    int dist_gibbs_marginals_many(
        dist_gibbs_t * const *, size_t, size_t, const uint32_t * const *,
        const uint32_t *, size_t, float *, float *, size_t, float *) nogil
    int dist_gibbs_relate(dist_gibbs_t *, size_t, uint32_t, uint32_t,
                          uint64_t, double *, double *, double *) nogil
    int dist_gibbs_relate_many(dist_gibbs_t * const *, size_t, size_t,
                               uint32_t, uint32_t, uint64_t, double *,
                               double *, double *) nogil
    size_t dist_gibbs_group_count(const dist_gibbs_t *)
    size_t dist_gibbs_row_count(const dist_gibbs_t *)
    int dist_gibbs_counts(const dist_gibbs_t *, int *)
    int dist_gibbs_assignments(const dist_gibbs_t *, uint32_t *)
    int dist_gibbs_get_group(const dist_gibbs_t *, int, size_t, uint32_t *)
    int dist_gibbs_packed_to_global(const dist_gibbs_t *, uint32_t, uint32_t *)
    int dist_gibbs_global_to_packed(const dist_gibbs_t *, uint32_t, uint32_t *)
    size_t dist_gibbs_global_size(const dist_gibbs_t *)
    int dist_gibbs_debug_counts(dist_gibbs_t *, uint64_t *, size_t)
    ctypedef struct dist_validate_report_t:
        int code
        int feature
        long long group
        long long detail
        long long expected
        long long found
        long long rows_assigned
        char what[96]
    int dist_gibbs_validate(dist_gibbs_t *, dist_validate_report_t *)
    int dist_gibbs_comm_stats(dist_gibbs_t *, double *, uint64_t *, int)
    int dist_gibbs_phase_stats(dist_gibbs_t *, double *, uint64_t *, int)
    size_t dist_gibbs_float_delta_words(const dist_gibbs_t *)
    int dist_gibbs_batch_float_delta_dev(dist_gibbs_t *, double *)
    int dist_gibbs_batch_apply_float_delta_dev(dist_gibbs_t *, const double *)
    int dist_gibbs_export_float_moments_dev(dist_gibbs_t *, double *)
    int dist_gibbs_import_float_moments_dev(dist_gibbs_t *, const double *)
    int dist_gibbs_sharded_device_normalise_ok(const dist_gibbs_t *, size_t,
                                               size_t, int *)
    int dist_gibbs_kernel_stats(dist_gibbs_t *, double *, uint64_t *,
                                uint64_t *, int)
    int dist_gibbs_set_option(dist_gibbs_t *, const char *, int)
    int dist_gibbs_set_certified_search(dist_gibbs_t *, int, int)
    int dist_gibbs_path_counts(const dist_gibbs_t *, uint64_t *, uint64_t *)
    int dist_gibbs_shared(const dist_gibbs_t *, int, dist_shared_t *)
    int dist_gibbs_clustering(const dist_gibbs_t *, float *, float *)
    int dist_gibbs_score_data(dist_gibbs_t *, float *, float *)
    int dist_gibbs_score_data_grid(dist_gibbs_t *, int, const dist_shared_t *,
                                   size_t, float *)
    int dist_gibbs_score_counts_grid(dist_gibbs_t *, const float *,
                                     const float *, size_t, float *)
    int dist_gibbs_set_shared(dist_gibbs_t *, int, const dist_shared_t *)
    int dist_gibbs_set_clustering(dist_gibbs_t *, float, float)
    int dist_gibbs_sample_hypers(dist_gibbs_t *, int, const dist_shared_t *,
                                 size_t, uint32_t *, size_t *)
    int dist_gibbs_sample_clustering(dist_gibbs_t *, const float *,
                                     const float *, size_t, uint32_t *,
                                     size_t *)
    int dist_gibbs_sample_hypers_pass(dist_gibbs_t *, int, const int *,
                                      size_t, const float *, size_t, size_t,
                                      uint32_t *, uint32_t *)
    int dist_gibbs_sample_hypers_pass_many(dist_gibbs_t * const *, size_t,
                                           int, const int *, size_t,
                                           const float *, size_t, size_t,
                                           uint32_t *, uint32_t *)
    int dist_gibbs_hyper_stats(dist_gibbs_t *, uint64_t *)


PREDICT_FEATURE_RECOMPUTE = 1   # DIST_PREDICT_FEATURE_RECOMPUTE
PREDICT_MANY_DRAW_ALL = 1       # DIST_PREDICT_MANY_DRAW_ALL
KIND_DD = DIST_DD
KIND_BB = DIST_BB
KIND_GP = DIST_GP
KIND_NICH = DIST_NICH
KIND_DPD = DIST_DPD
KIND_BNB = DIST_BNB
DPD_OTHER = 0xFFFFFFFF


cdef inline int check(int rc) except -1:
    if rc != 0:
        raise RuntimeError(dist_last_error().decode("utf-8", "replace"))
    return 0


cdef inline object checked_size(size_t n):
    # the size_t getters report a failure as (size_t)-1
    if n == <size_t> -1:
        raise RuntimeError(dist_last_error().decode("utf-8", "replace"))
    return n


def abi_version():
    return dist_abi_version()


def device_count():
    cdef int n = 0
    check(dist_device_count(&n))
    return n


def set_device(int device):
    check(dist_set_device(device))


def synchronize():
    check(dist_synchronize())


def set_stream(size_t hip_stream):
    """the calling thread's HIP stream (0 = default), e.g.
    torch.cuda.Stream().cuda_stream"""
    check(dist_set_stream(<void *> hip_stream))


# ---------------------------------------------------------------------------
# Shared: the hyper-parameters of one feature

cdef class SharedParams:
    """dist_shared_t plus the storage it points at."""
    cdef dist_shared_t c
    cdef object _betas

    def __cinit__(self):
        memset(&self.c, 0, sizeof(dist_shared_t))
        self._betas = None

    @staticmethod
    def make(int kind, p=(), alphas=(), betas=None):
        cdef SharedParams s = SharedParams()
        cdef int i
        cdef cnp.ndarray[cnp.float32_t, ndim=1] b
        s.c.kind = kind
        for i in range(len(p)):
            s.c.p[i] = p[i]
        if kind == DIST_DD:
            if not 1 <= len(alphas) <= 256:
                raise RuntimeError("expected 1 <= dim <= 256")
            s.c.dim = len(alphas)
            for i in range(len(alphas)):
                s.c.alphas[i] = alphas[i]
        if kind == DIST_DPD:
            b = np.ascontiguousarray(betas, dtype=np.float32)
            s._betas = b
            s.c.dim = b.shape[0]
            s.c.betas = <const float *> b.data
        return s

    property kind:
        def __get__(self):
            return self.c.kind

    property dim:
        def __get__(self):
            return self.c.dim

    property p:
        def __get__(self):
            return [self.c.p[i] for i in range(4)]

    property alphas:
        def __get__(self):
            return [self.c.alphas[i] for i in range(self.c.dim)]

    property betas:
        def __get__(self):
            return None if self._betas is None else self._betas.copy()

    def group_words(self):
        return dist_group_words(&self.c)

    # Model::Group scalar operations on a words array
    def group_init(self):
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] g = np.zeros(
            self.group_words(), np.uint32)
        check(dist_group_init(&self.c, <uint32_t *> g.data))
        return g

    def group_add_value(self, cnp.ndarray[cnp.uint32_t, ndim=1] g,
                        uint32_t value):
        check(dist_group_add_value(&self.c, <uint32_t *> g.data, value))

    def group_remove_value(self, cnp.ndarray[cnp.uint32_t, ndim=1] g,
                           uint32_t value):
        check(dist_group_remove_value(&self.c, <uint32_t *> g.data, value))

    def group_score_value(self, cnp.ndarray[cnp.uint32_t, ndim=1] g,
                          uint32_t value):
        cdef float out = 0
        check(dist_group_score_value(&self.c, <const uint32_t *> g.data, value,
                                     &out))
        return out

    def group_sample_value(self, cnp.ndarray[cnp.uint32_t, ndim=1] g,
                           uint32_t seed_state, row_first, size_t n,
                           int feature):
        """n draws from the group's posterior predictive
        (dist_group_sample_value): the words of cells (row_first + i,
        feature) under seed_state.  -> uint32 words"""
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] out = np.zeros(n, np.uint32)
        cdef uint64_t r0 = <uint64_t> row_first
        cdef int rc
        with nogil:
            rc = dist_group_sample_value(&self.c, <const uint32_t *> g.data,
                                         seed_state, r0, n, feature,
                                         <uint32_t *> out.data)
        check(rc)
        return out

    def group_score_data(self, cnp.ndarray[cnp.uint32_t, ndim=1] g):
        cdef float out = 0
        check(dist_group_score_data(&self.c, <const uint32_t *> g.data, &out))
        return out

    # Model::Scorer (dd.hpp:222-245 and the other models'): init -> state
    def scorer_init(self, cnp.ndarray[cnp.uint32_t, ndim=1] g):
        cdef cnp.ndarray[cnp.float32_t, ndim=1] state = np.zeros(
            dist_scorer_words(&self.c), np.float32)
        check(dist_scorer_init(&self.c, <const uint32_t *> g.data,
                               <float *> state.data))
        return state

    def scorer_eval(self, cnp.ndarray[cnp.float32_t, ndim=1] state,
                    uint32_t value):
        cdef float out = 0
        check(dist_scorer_eval(&self.c, <const float *> state.data, value,
                               &out))
        return out

    # protobuf wire bytes (schema.proto messages) without libprotobuf
    def group_protobuf_dump(self, cnp.ndarray[cnp.uint32_t, ndim=1] g,
                            keys=None):
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] k
        cdef const uint32_t * kp = NULL
        if keys is not None:
            k = np.ascontiguousarray(keys, np.uint32)
            kp = <const uint32_t *> k.data
        cdef size_t n = 0
        check(dist_group_protobuf_dump(&self.c, <const uint32_t *> g.data, kp,
                                       NULL, 0, &n))
        cdef cnp.ndarray[cnp.uint8_t, ndim=1] buf = np.zeros(max(n, 1),
                                                            np.uint8)
        check(dist_group_protobuf_dump(&self.c, <const uint32_t *> g.data, kp,
                                       <uint8_t *> buf.data, n, &n))
        return buf[:n].tobytes()

    def group_protobuf_load(self, bytes data, keys=None):
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] k
        cdef const uint32_t * kp = NULL
        if keys is not None:
            k = np.ascontiguousarray(keys, np.uint32)
            kp = <const uint32_t *> k.data
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] g = np.zeros(
            self.group_words(), np.uint32)
        cdef const unsigned char * d = data
        check(dist_group_protobuf_load(&self.c, kp, <const uint8_t *> d,
                                       len(data), <uint32_t *> g.data))
        return g

    def protobuf_dump(self):
        cdef size_t n = 0
        check(dist_shared_protobuf_dump(&self.c, NULL, 0, &n))
        cdef cnp.ndarray[cnp.uint8_t, ndim=1] buf = np.zeros(max(n, 1),
                                                            np.uint8)
        check(dist_shared_protobuf_dump(&self.c, <uint8_t *> buf.data, n, &n))
        return buf[:n].tobytes()

    @staticmethod
    def protobuf_load(int kind, bytes data):
        cdef SharedParams s = SharedParams()
        cdef const unsigned char * d = data
        check(dist_shared_protobuf_load(kind, <const uint8_t *> d, len(data),
                                        &s.c))
        return s


# ---------------------------------------------------------------------------
# entropy and sampling

cdef class DpdShared:
    """DirichletProcessDiscrete::Shared's stick-breaking state
    (dist_dpd_shared_t; dpd.hpp:59-124)"""
    cdef dist_dpd_shared_t * h

    def __cinit__(self):
        self.h = dist_dpd_shared_create()
        if self.h == NULL:
            raise MemoryError()

    def __dealloc__(self):
        if self.h != NULL:
            dist_dpd_shared_destroy(self.h)
            self.h = NULL

    def load(self, float gamma, float alpha, values, betas, counts):
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] v = np.ascontiguousarray(
            values, dtype=np.uint32)
        cdef cnp.ndarray[cnp.float32_t, ndim=1] b = np.ascontiguousarray(
            betas, dtype=np.float32)
        cdef cnp.ndarray[cnp.int32_t, ndim=1] c = np.ascontiguousarray(
            counts, dtype=np.int32)
        if not (v.shape[0] == b.shape[0] == c.shape[0]):
            raise RuntimeError("invalid message")
        check(dist_dpd_shared_load(self.h, gamma, alpha,
                                   <const uint32_t *> v.data,
                                   <const float *> b.data,
                                   <const int *> c.data, v.shape[0]))

    def add_value(self, uint32_t value, uint32_t rng_state):
        check(dist_dpd_shared_add_value(self.h, value, &rng_state))
        return rng_state

    def remove_value(self, uint32_t value):
        check(dist_dpd_shared_remove_value(self.h, value))

    def realize(self, uint32_t rng_state):
        check(dist_dpd_shared_realize(self.h, &rng_state))
        return rng_state

    def slot(self, uint32_t value):
        cdef uint32_t out = 0
        check(dist_dpd_shared_slot(self.h, value, &out))
        return out

    def __len__(self):
        return dist_dpd_shared_size(self.h)

    property slots:
        def __get__(self):
            return dist_dpd_shared_slots(self.h)

    property version:
        def __get__(self):
            return dist_dpd_shared_version(self.h)

    def scalars(self):
        """(gamma, alpha, beta0)"""
        cdef float g = 0, a = 0, b = 0
        check(dist_dpd_shared_params(self.h, &g, &a, &b))
        return g, a, b

    def dump(self):
        """by dense slot: values (0xFFFFFFFF = free), betas, counts"""
        cdef size_t n = dist_dpd_shared_slots(self.h)
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] v = np.zeros(n, np.uint32)
        cdef cnp.ndarray[cnp.float32_t, ndim=1] b = np.zeros(n, np.float32)
        cdef cnp.ndarray[cnp.int32_t, ndim=1] c = np.zeros(n, np.int32)
        check(dist_dpd_shared_dump(self.h, <uint32_t *> v.data,
                                   <float *> b.data, <int *> c.data))
        return v, b, c

    def params(self):
        """the SharedParams (dist_shared_t) mixtures and groups take: a
        snapshot (betas copied) of the dense view"""
        cdef dist_shared_t view
        check(dist_dpd_shared_view(self.h, &view))
        v, b, c = self.dump()
        return SharedParams.make(DIST_DPD, p=(view.p[0], view.p[1]), betas=b)


def sample_gamma(uint32_t rng_state, float alpha, float beta=1.0):
    """random.hpp:87-97 -> (draw, engine state after)"""
    cdef float out = 0
    check(dist_sample_gamma(&rng_state, alpha, beta, &out))
    return out, rng_state


def sample_beta_safe(uint32_t rng_state, float alpha, float beta,
                     float min_value):
    """random.hpp:110-119 -> (draw, engine state after)"""
    cdef float out = 0
    check(dist_sample_beta_safe(&rng_state, alpha, beta, min_value, &out))
    return out, rng_state


def rng_seed(seed):
    return dist_rng_seed(<uint64_t> seed)


def rng_next(uint32_t state):
    """-> (raw engine output == new state)"""
    cdef uint32_t s = state
    dist_rng_next(&s)
    return s


def rng_unif01(uint32_t state):
    """-> (u, new state)"""
    cdef uint32_t s = state
    cdef float u = dist_rng_unif01(&s)
    return u, s


def rng_jump(uint32_t state, steps):
    return dist_rng_jump(state, <uint64_t> steps)


def _vector(int op, x):
    cdef cnp.ndarray[cnp.float32_t, ndim=1] a
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] u
    cdef cnp.ndarray[cnp.float32_t, ndim=1] out
    if op == 4:
        u = np.ascontiguousarray(x, dtype=np.uint32)
        out = np.zeros(u.shape[0], np.float32)
        check(dist_vector_log_factorial(u.shape[0], <const uint32_t *> u.data,
                                        <float *> out.data))
        return out
    a = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros(a.shape[0], np.float32)
    if op == 0:
        check(dist_vector_log(a.shape[0], <const float *> a.data, <float *> out.data))
    elif op == 1:
        check(dist_vector_exp(a.shape[0], <const float *> a.data, <float *> out.data))
    elif op == 2:
        check(dist_vector_lgamma(a.shape[0], <const float *> a.data, <float *> out.data))
    else:
        check(dist_vector_lgamma_nu(a.shape[0], <const float *> a.data, <float *> out.data))
    return out


def vector_log(x):
    return _vector(0, x)


def vector_exp(x):
    return _vector(1, x)


def vector_lgamma(x):
    return _vector(2, x)


def vector_lgamma_nu(x):
    return _vector(3, x)


def vector_log_factorial(x):
    return _vector(4, x)


def sample_from_scores_overwrite(uint32_t state,
                                 cnp.ndarray[cnp.float32_t, ndim=1] scores):
    """-> (sample, new state); scores become likelihoods in place"""
    cdef uint32_t s = state
    cdef size_t sample = 0
    check(dist_sample_from_scores_overwrite(&s, scores.shape[0],
                                            <float *> scores.data, &sample))
    return sample, s


def scores_to_likelihoods(cnp.ndarray[cnp.float32_t, ndim=1] scores):
    cdef float total = 0
    check(dist_scores_to_likelihoods(scores.shape[0], <float *> scores.data,
                                     &total))
    return total


def sample_from_likelihoods(uint32_t state,
                            cnp.ndarray[cnp.float32_t, ndim=1] likelihoods,
                            float total):
    cdef uint32_t s = state
    cdef size_t sample = 0
    check(dist_sample_from_likelihoods(&s, likelihoods.shape[0],
                                       <const float *> likelihoods.data, total,
                                       &sample))
    return sample, s


def log_sum_exp(scores):
    cdef cnp.ndarray[cnp.float32_t, ndim=1] a = np.ascontiguousarray(
        scores, dtype=np.float32)
    cdef float out = 0
    check(dist_log_sum_exp(a.shape[0], <const float *> a.data, &out))
    return out


def py_score_add_value(float alpha, float d, int group_size,
                       int nonempty_group_count, int sample_size,
                       int empty_group_count=1):
    cdef float out = 0
    check(dist_py_score_add_value(alpha, d, group_size, nonempty_group_count,
                                  sample_size, empty_group_count, &out))
    return out


def py_score_remove_value(float alpha, float d, int group_size,
                          int nonempty_group_count, int sample_size,
                          int empty_group_count=1):
    cdef float out = 0
    check(dist_py_score_remove_value(alpha, d, group_size,
                                     nonempty_group_count, sample_size,
                                     empty_group_count, &out))
    return out


def py_sample_assignments(float alpha, float d, int size, uint32_t state):
    """-> (assignments, new rng state)"""
    cdef cnp.ndarray[cnp.int32_t, ndim=1] out = np.zeros(max(size, 1),
                                                         np.int32)
    cdef uint32_t s = state
    check(dist_py_sample_assignments(alpha, d, size, &s, <int *> out.data))
    return out[:size], s


def py_score_counts(float alpha, float d, counts):
    cdef cnp.ndarray[cnp.int32_t, ndim=1] c = np.ascontiguousarray(
        counts, dtype=np.int32)
    cdef float out = 0
    check(dist_py_score_counts(alpha, d, <const int *> c.data, c.shape[0],
                               &out))
    return out


# ---------------------------------------------------------------------------
# PitmanYor::Mixture

cdef class PyMixture:
    cdef dist_py_mixture_t * ptr

    def __cinit__(self):
        self.ptr = dist_py_mixture_create()
        if self.ptr == NULL:
            raise RuntimeError(dist_last_error().decode())

    def __dealloc__(self):
        if self.ptr != NULL:
            dist_py_mixture_destroy(self.ptr)

    def __len__(self):
        return dist_py_mixture_size(self.ptr)

    def init(self, float alpha, float d, counts):
        cdef cnp.ndarray[cnp.int32_t, ndim=1] c = np.ascontiguousarray(
            counts, dtype=np.int32)
        check(dist_py_mixture_init(self.ptr, alpha, d, <const int *> c.data,
                                   c.shape[0]))

    def add_value(self, float alpha, float d, size_t groupid):
        cdef int added = 0
        check(dist_py_mixture_add_value(self.ptr, alpha, d, groupid, &added))
        return bool(added)

    def remove_value(self, float alpha, float d, size_t groupid):
        cdef int removed = 0
        check(dist_py_mixture_remove_value(self.ptr, alpha, d, groupid,
                                           &removed))
        return bool(removed)

    def score_value(self, float alpha, float d,
                    cnp.ndarray[cnp.float32_t, ndim=1] scores):
        check(dist_py_mixture_score_value(self.ptr, alpha, d,
                                          <float *> scores.data,
                                          scores.shape[0]))

    def score_data(self, float alpha, float d):
        cdef float out = 0
        check(dist_py_mixture_score_data(self.ptr, alpha, d, &out))
        return out

    def sample_size(self):
        return dist_py_mixture_sample_size(self.ptr)

    def counts(self):
        cdef cnp.ndarray[cnp.int32_t, ndim=1] out = np.zeros(len(self),
                                                            np.int32)
        if len(self):
            check(dist_py_mixture_counts(self.ptr, <int *> out.data))
        return out

    def empty_groupids(self):
        cdef size_t n = dist_py_mixture_empty_groupids(self.ptr, NULL, 0)
        cdef size_t * buf = <size_t *> malloc(sizeof(size_t) * (n + 1))
        dist_py_mixture_empty_groupids(self.ptr, buf, n)
        out = [buf[i] for i in range(n)]
        free(buf)
        return out


# ---------------------------------------------------------------------------
# Clustering<int>::LowEntropy

def le_score_add_value(int dataset_size, int group_size, int nonempty,
                       int sample_size, int empty=1):
    cdef float out = 0
    check(dist_le_score_add_value(dataset_size, group_size, nonempty,
                                  sample_size, empty, &out))
    return out


def le_score_remove_value(int dataset_size, int group_size, int nonempty,
                          int sample_size, int empty=1):
    cdef float out = 0
    check(dist_le_score_remove_value(dataset_size, group_size, nonempty,
                                     sample_size, empty, &out))
    return out


def le_log_partition_function(int sample_size):
    cdef float out = 0
    check(dist_le_log_partition_function(sample_size, &out))
    return out


def le_sample_assignments(int dataset_size, int size, uint32_t rng_state):
    """-> (int32 assignments, new rng state)"""
    cdef cnp.ndarray[cnp.int32_t, ndim=1] out = np.zeros(max(size, 1), np.int32)
    cdef uint32_t s = rng_state
    check(dist_le_sample_assignments(dataset_size, size, &s, <int *> out.data))
    return out[:size], s


def le_score_counts(int dataset_size, counts):
    cdef cnp.ndarray[cnp.int32_t, ndim=1] c = np.ascontiguousarray(
        counts, dtype=np.int32)
    cdef float out = 0
    check(dist_le_score_counts(dataset_size, <const int *> c.data, c.shape[0],
                               &out))
    return out


cdef class LeMixture:
    cdef dist_le_mixture_t * ptr

    def __cinit__(self):
        self.ptr = dist_le_mixture_create()
        if self.ptr == NULL:
            raise RuntimeError(dist_last_error().decode())

    def __dealloc__(self):
        if self.ptr != NULL:
            dist_le_mixture_destroy(self.ptr)

    def __len__(self):
        return dist_le_mixture_size(self.ptr)

    def init(self, counts):
        cdef cnp.ndarray[cnp.int32_t, ndim=1] c = np.ascontiguousarray(
            counts, dtype=np.int32)
        check(dist_le_mixture_init(self.ptr, <const int *> c.data, c.shape[0]))

    def add_value(self, size_t groupid):
        cdef int added = 0
        check(dist_le_mixture_add_value(self.ptr, groupid, &added))
        return bool(added)

    def remove_value(self, size_t groupid):
        cdef int removed = 0
        check(dist_le_mixture_remove_value(self.ptr, groupid, &removed))
        return bool(removed)

    def score_value(self, int dataset_size,
                    cnp.ndarray[cnp.float32_t, ndim=1] scores):
        check(dist_le_mixture_score_value(self.ptr, dataset_size,
                                          <float *> scores.data,
                                          scores.shape[0]))

    def score_data(self, int dataset_size):
        cdef float out = 0
        check(dist_le_mixture_score_data(self.ptr, dataset_size, &out))
        return out

    def sample_size(self):
        return dist_le_mixture_sample_size(self.ptr)

    def counts(self):
        cdef cnp.ndarray[cnp.int32_t, ndim=1] out = np.zeros(len(self),
                                                            np.int32)
        if len(self):
            check(dist_le_mixture_counts(self.ptr, <int *> out.data))
        return out

    def empty_groupids(self):
        return [i for i, c in enumerate(self.counts()) if c == 0]


# ---------------------------------------------------------------------------
# Model::Mixture

cdef class SlaveMixture:
    cdef dist_mixture_t * ptr
    cdef SharedParams shared

    def __cinit__(self, SharedParams shared):
        self.shared = shared
        self.ptr = dist_mixture_create(&shared.c)
        if self.ptr == NULL:
            raise RuntimeError(dist_last_error().decode())

    def __dealloc__(self):
        if self.ptr != NULL:
            dist_mixture_destroy(self.ptr)

    def __len__(self):
        return dist_mixture_size(self.ptr)

    def clear(self):
        check(dist_mixture_clear(self.ptr))

    def append(self, cnp.ndarray[cnp.uint32_t, ndim=1] group):
        if group.shape[0] != <Py_ssize_t> self.shared.group_words():
            raise RuntimeError("group has the wrong size")
        check(dist_mixture_append(self.ptr, <const uint32_t *> group.data))

    def get_group(self, size_t groupid):
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] g = np.zeros(
            self.shared.group_words(), np.uint32)
        check(dist_mixture_get_group(self.ptr, groupid, <uint32_t *> g.data))
        return g

    def init(self):
        check(dist_mixture_init(self.ptr))

    def add_group(self):
        check(dist_mixture_add_group(self.ptr))

    def remove_group(self, size_t groupid):
        check(dist_mixture_remove_group(self.ptr, groupid))

    def add_value(self, size_t groupid, uint32_t value):
        check(dist_mixture_add_value(self.ptr, groupid, value))

    def remove_value(self, size_t groupid, uint32_t value):
        check(dist_mixture_remove_value(self.ptr, groupid, value))

    def score_value_group(self, size_t groupid, uint32_t value):
        cdef float out = 0
        check(dist_mixture_score_value_group(self.ptr, groupid, value, &out))
        return out

    def score_value(self, uint32_t value,
                    cnp.ndarray[cnp.float32_t, ndim=1] scores_accum):
        check(dist_mixture_score_value(self.ptr, value,
                                       <float *> scores_accum.data,
                                       scores_accum.shape[0]))

    def score_data(self):
        cdef float out = 0
        check(dist_mixture_score_data(self.ptr, &out))
        return out

    def score_values(self, values,
                     cnp.ndarray[cnp.float32_t, ndim=2, mode="c"] scores_accum):
        """score_value for len(values) values in one launch:
        scores_accum[r, k] accumulates (dist_mixture_score_values)"""
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] v = np.ascontiguousarray(
            values, dtype=np.uint32)
        if scores_accum.shape[0] != v.shape[0]:
            raise RuntimeError("scores_accum has one row per value")
        check(dist_mixture_score_values(self.ptr, <const uint32_t *> v.data,
                                        v.shape[0],
                                        <float *> scores_accum.data,
                                        scores_accum.shape[1]))

    def validate(self):
        """Mixture::validate (mixture.hpp:440-444): raises RuntimeError"""
        check(dist_mixture_validate(self.ptr))

    def score_data_grid(self, shareds):
        """shareds: SharedParams candidates -> float32 scores, one each"""
        cdef size_t n = len(shareds)
        cdef cnp.ndarray[cnp.float32_t, ndim=1] out = np.zeros(n, np.float32)
        if n == 0:
            return out
        cdef dist_shared_t * arr = <dist_shared_t *> malloc(
            n * sizeof(dist_shared_t))
        cdef SharedParams s
        for i in range(n):
            s = shareds[i]
            arr[i] = s.c
        cdef int rc = dist_mixture_score_data_grid(self.ptr, arr, n,
                                                   <float *> out.data)
        free(arr)
        check(rc)
        return out


# ---------------------------------------------------------------------------
# MixtureIdTracker

cdef class IdTracker:
    cdef dist_id_tracker_t * ptr

    def __cinit__(self):
        self.ptr = dist_id_tracker_create()

    def __dealloc__(self):
        if self.ptr != NULL:
            dist_id_tracker_destroy(self.ptr)

    def init(self, size_t group_count=0):
        check(dist_id_tracker_init(self.ptr, group_count))

    def add_group(self):
        check(dist_id_tracker_add_group(self.ptr))

    def remove_group(self, uint32_t packed):
        check(dist_id_tracker_remove_group(self.ptr, packed))

    def packed_to_global(self, uint32_t packed):
        cdef uint32_t out = 0
        check(dist_id_tracker_packed_to_global(self.ptr, packed, &out))
        return out

    def global_to_packed(self, uint32_t global_):
        cdef uint32_t out = 0
        check(dist_id_tracker_global_to_packed(self.ptr, global_, &out))
        return out

    def packed_size(self):
        return dist_id_tracker_packed_size(self.ptr)

    def global_size(self):
        return dist_id_tracker_global_size(self.ptr)


# ---------------------------------------------------------------------------
# the batched row engine

def value_words(int kind, values):
    """Values of one feature as the 32-bit words the ABI takes."""
    if kind == DIST_NICH:
        return np.ascontiguousarray(values, dtype=np.float32).view(np.uint32)
    return np.ascontiguousarray(values).astype(np.uint32)


def comm_available():
    """True if RCCL can be bound at run time"""
    return bool(dist_comm_available())


def comm_unique_id():
    """128 bytes for rank 0 to hand to the other ranks"""
    cdef cnp.ndarray[cnp.uint8_t, ndim=1] out = np.zeros(128, np.uint8)
    check(dist_comm_unique_id(<uint8_t *> out.data))
    return out


def comm_unique_id_host():
    """128 bytes naming a host (shared-memory) communicator: ranks that share
    one GPU, where RCCL cannot be used"""
    cdef cnp.ndarray[cnp.uint8_t, ndim=1] out = np.zeros(128, np.uint8)
    check(dist_comm_unique_id_host(<uint8_t *> out.data))
    return out


cdef class Comm:
    """the library's own communicator (collective constructor): RCCL, or the
    host transport when the id came from comm_unique_id_host()"""
    cdef dist_comm_t * ptr

    def __cinit__(self, unique_id, int rank, int world):
        cdef cnp.ndarray[cnp.uint8_t, ndim=1] uid = np.ascontiguousarray(
            unique_id, dtype=np.uint8)
        if uid.shape[0] != 128:
            raise ValueError("the unique id is 128 bytes")
        cdef const uint8_t * p = <const uint8_t *> uid.data
        with nogil:
            self.ptr = dist_comm_create(p, rank, world)
        if self.ptr == NULL:
            raise RuntimeError(dist_last_error().decode())

    def __dealloc__(self):
        if self.ptr != NULL:
            dist_comm_destroy(self.ptr)

    def size(self):
        """-> (rank, world)"""
        cdef int r = 0, w = 0
        check(dist_comm_size(self.ptr, &r, &w))
        return r, w

    def all_reduce_dev(self, size_t ptr, size_t count, dtype="int32",
                       op="sum"):
        """in place, on device memory; waited for"""
        cdef int t = {"int32": 0, "float64": 1}[dtype]
        cdef int o = {"sum": 0, "min": 1}[op]
        cdef int rc
        with nogil:
            rc = dist_comm_all_reduce_dev(self.ptr, <void *> ptr, count, t, o)
        check(rc)


cdef class GibbsEngine:
    cdef dist_gibbs_t * ptr
    cdef list shareds
    cdef object _keep   # device tensors / arrays the engine points into

    def __cinit__(self, float alpha, float d, shareds, dataset_size=None):
        """dataset_size: the LowEntropy clustering model instead of
        PitmanYor(alpha, d)"""
        cdef int n = len(shareds)
        cdef dist_shared_t * arr = <dist_shared_t *> malloc(
            sizeof(dist_shared_t) * (n + 1))
        cdef SharedParams s
        cdef int i
        for i in range(n):
            s = shareds[i]
            memcpy(&arr[i], &s.c, sizeof(dist_shared_t))
        self.shareds = list(shareds)
        if dataset_size is None:
            self.ptr = dist_gibbs_create(alpha, d, n, arr)
        else:
            self.ptr = dist_gibbs_create_low_entropy(int(dataset_size), n, arr)
        free(arr)
        if self.ptr == NULL:
            raise RuntimeError(dist_last_error().decode())

    def __dealloc__(self):
        if self.ptr != NULL:
            dist_gibbs_destroy(self.ptr)

    def load_rows(self, values, assign_packed, int nonempty_groups,
                  int empty_groups=1, row_offset=0):
        """values: one host array per feature; assign_packed: host uint32."""
        cdef int n = len(self.shareds)
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] a = np.ascontiguousarray(
            assign_packed, dtype=np.uint32)
        cdef const uint32_t ** ptrs = <const uint32_t **> malloc(
            sizeof(void *) * (n + 1))
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] w
        cdef SharedParams s
        words = []
        cdef int i
        for i in range(n):
            s = self.shareds[i]
            w = value_words(s.c.kind, values[i])
            if w.shape[0] != a.shape[0]:
                free(ptrs)
                raise RuntimeError("feature columns differ in length")
            words.append(w)
            ptrs[i] = <const uint32_t *> w.data
        cdef int rc = dist_gibbs_load_rows(self.ptr, a.shape[0], ptrs,
                                           <const uint32_t *> a.data,
                                           nonempty_groups, empty_groups,
                                           <uint64_t> row_offset)
        free(ptrs)
        check(rc)

    def load_rows_unassigned(self, values, int empty_groups=1, row_offset=0):
        """rows without a group yet; init_sequential assigns them"""
        cdef int n = len(self.shareds)
        cdef const uint32_t ** ptrs = <const uint32_t **> malloc(
            sizeof(void *) * (n + 1))
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] w
        cdef SharedParams s
        words = []
        cdef int i
        cdef size_t rows = 0
        for i in range(n):
            s = self.shareds[i]
            w = value_words(s.c.kind, values[i])
            if i and w.shape[0] != rows:
                free(ptrs)
                raise RuntimeError("feature columns differ in length")
            rows = w.shape[0]
            words.append(w)
            ptrs[i] = <const uint32_t *> w.data
        cdef int rc = dist_gibbs_load_rows_unassigned(
            self.ptr, rows, ptrs, empty_groups, <uint64_t> row_offset)
        free(ptrs)
        check(rc)

    def init_sequential(self, size_t row_begin, size_t row_end,
                        uint32_t rng_state, prior_only=False):
        """-> new rng state"""
        cdef uint32_t s = rng_state
        cdef int rc
        cdef int prior = 1 if prior_only else 0
        with nogil:
            rc = dist_gibbs_init_sequential(self.ptr, row_begin, row_end, &s,
                                            prior)
        check(rc)
        return s

    def load_rows_dev(self, value_ptrs, size_t assign_ptr, size_t n_rows,
                      int nonempty_groups, int empty_groups=1, row_offset=0,
                      keep=None):
        """Device pointers (e.g. torch tensor data_ptr()); `keep` holds the
        owners alive for the lifetime of the engine."""
        cdef int n = len(self.shareds)
        cdef const uint32_t ** ptrs = <const uint32_t **> malloc(
            sizeof(void *) * (n + 1))
        cdef int i
        cdef size_t addr
        for i in range(n):
            addr = value_ptrs[i]
            ptrs[i] = <const uint32_t *> addr
        self._keep = keep
        cdef int rc = dist_gibbs_load_rows_dev(
            self.ptr, n_rows, ptrs, <uint32_t *> assign_ptr, nonempty_groups,
            empty_groups, <uint64_t> row_offset)
        free(ptrs)
        check(rc)

    def stat_words(self):
        return checked_size(dist_gibbs_stat_words(self.ptr))

    def export_stats_dev(self, size_t ptr):
        check(dist_gibbs_export_stats_dev(self.ptr, <int32_t *> ptr))

    def import_stats_dev(self, size_t ptr):
        check(dist_gibbs_import_stats_dev(self.ptr, <const int32_t *> ptr))

    def sweep(self, size_t row_begin, size_t row_end, size_t batch_rows,
              uint32_t seed_state, draw_base=0):
        cdef uint64_t db = <uint64_t> draw_base
        cdef int rc
        with nogil:
            rc = dist_gibbs_sweep(self.ptr, row_begin, row_end, batch_rows,
                                  seed_state, db)
        check(rc)

    def sweep_sequential(self, size_t row_begin, size_t row_end,
                         uint32_t rng_state):
        """-> new rng state"""
        cdef uint32_t s = rng_state
        cdef int rc
        with nogil:
            rc = dist_gibbs_sweep_sequential(self.ptr, row_begin, row_end, &s)
        check(rc)
        return s

    def sweep_sharded(self, Comm comm, size_t n_batches, size_t batch_rows,
                      uint32_t seed_state, draw_base=0):
        cdef uint64_t db = <uint64_t> draw_base
        cdef int rc
        with nogil:
            rc = dist_gibbs_sweep_sharded(self.ptr, comm.ptr, n_batches,
                                          batch_rows, seed_state, db)
        check(rc)

    def partition_by_value(self, Comm comm):
        """collective: no value has rows on two ranks -> sweep_sharded
        exchanges 3 words per group instead of the cells"""
        cdef int rc
        with nogil:
            rc = dist_gibbs_partition_by_value(self.ptr, comm.ptr)
        check(rc)

    def gather_cells(self, Comm comm):
        """collective: make a value-partitioned replica whole again"""
        cdef int rc
        with nogil:
            rc = dist_gibbs_gather_cells(self.ptr, comm.ptr)
        check(rc)

    def comm_volume(self, reset=False):
        """-> dict: all-reduces of sweep_sharded, int32 words sent in all,
        the largest, the last"""
        cdef uint64_t v[4]
        check(dist_gibbs_comm_volume(self.ptr, v, 1 if reset else 0))
        return {"collectives": int(v[0]), "words": int(v[1]),
                "words_max": int(v[2]), "words_last": int(v[3])}

    def batch_sample(self, size_t row_begin, size_t row_end,
                     uint32_t seed_state, draw_base=0):
        check(dist_gibbs_batch_sample(self.ptr, row_begin, row_end, seed_state,
                                      <uint64_t> draw_base))

    def batch_delta_dev(self, size_t ptr):
        check(dist_gibbs_batch_delta_dev(self.ptr, <int32_t *> ptr))

    def batch_apply_delta_dev(self, size_t ptr):
        check(dist_gibbs_batch_apply_delta_dev(self.ptr, <const int32_t *> ptr))

    def batch_apply_local(self):
        check(dist_gibbs_batch_apply_local(self.ptr))

    def ordered_features(self):
        """number of features with order-dependent statistics (NICH, GP)"""
        cdef int n = 0
        check(dist_gibbs_ordered_features(self.ptr, &n))
        return n

    def feature_is_ordered(self, int feature):
        cdef SharedParams s = self.shareds[feature]
        return s.c.kind == DIST_GP or s.c.kind == DIST_NICH

    def batch_moves_dev(self, size_t old_ptr, size_t new_ptr):
        check(dist_gibbs_batch_moves_dev(self.ptr, <uint32_t *> old_ptr,
                                         <uint32_t *> new_ptr))

    def replay_ordered_dev(self, size_t old_ptr, size_t new_ptr, value_ptrs,
                           size_t n_rows, bint reset):
        """value_ptrs: per feature a device address or 0"""
        cdef int n = len(value_ptrs)
        cdef const uint32_t ** ptrs = <const uint32_t **> malloc(
            max(n, 1) * sizeof(void *))
        cdef size_t addr
        for i in range(n):
            addr = value_ptrs[i]
            ptrs[i] = <const uint32_t *> addr
        cdef int rc = dist_gibbs_replay_ordered_dev(
            self.ptr, <const uint32_t *> old_ptr, <const uint32_t *> new_ptr,
            ptrs, n_rows, reset)
        free(ptrs)
        check(rc)

    def batch_finish(self):
        check(dist_gibbs_batch_finish(self.ptr))

    def row_scores(self, size_t row):
        cdef cnp.ndarray[cnp.float32_t, ndim=1] out = np.zeros(
            self.group_count() + 1, np.float32)
        cdef size_t n = 0
        check(dist_gibbs_row_scores(self.ptr, row, <float *> out.data, &n))
        return out[:n].copy()

    def score_rows_dev(self, size_t row_begin, size_t row_end, size_t ptr,
                       size_t ld):
        check(dist_gibbs_score_rows_dev(self.ptr, row_begin, row_end,
                                        <float *> ptr, ld))

    def predict_dev(self, value_ptrs, size_t n_rows, size_t logp_ptr,
                    size_t group_ptr, int mode, uint32_t seed_state,
                    draw_base=0):
        """Held-out rows (dist_gibbs_predict_dev): value_ptrs are device
        addresses of one column of n_rows words per feature, logp_ptr /
        group_ptr device addresses or 0.  -> log_sum_exp of the clustering
        model's scores alone"""
        cdef int n = len(self.shareds)
        if len(value_ptrs) != n:
            raise RuntimeError("one value column per feature")
        cdef const uint32_t ** ptrs = <const uint32_t **> malloc(
            sizeof(void *) * (n + 1))
        cdef int i
        cdef size_t addr
        for i in range(n):
            addr = value_ptrs[i]
            ptrs[i] = <const uint32_t *> addr
        cdef uint64_t db = <uint64_t> draw_base
        cdef float total = 0
        cdef int rc
        with nogil:
            rc = dist_gibbs_predict_dev(self.ptr, n_rows, ptrs,
                                        <float *> logp_ptr,
                                        <uint32_t *> group_ptr, mode,
                                        seed_state, db, &total)
        free(ptrs)
        check(rc)
        return total

    def predict(self, values, mode, uint32_t seed_state, draw_base=0):
        """Held-out rows from host arrays (dist_gibbs_predict): values is one
        array per feature; mode 0 draws, 1 takes the first maximum, None
        leaves the groups out.  -> (logp, groups or None, prior_total)"""
        cdef int n = len(self.shareds)
        if len(values) != n:
            raise RuntimeError("one value column per feature")
        cdef const uint32_t ** ptrs = <const uint32_t **> malloc(
            sizeof(void *) * (n + 1))
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] w
        cdef SharedParams s
        words = []
        cdef int i
        cdef size_t rows = 0
        for i in range(n):
            s = self.shareds[i]
            w = value_words(s.c.kind, values[i])
            if i and w.shape[0] != rows:
                free(ptrs)
                raise RuntimeError("feature columns differ in length")
            rows = w.shape[0]
            words.append(w)
            ptrs[i] = <const uint32_t *> w.data
        cdef cnp.ndarray[cnp.float32_t, ndim=1] logp = np.zeros(
            rows, np.float32)
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] group = np.zeros(
            rows, np.uint32)
        cdef uint32_t * gp = NULL if mode is None else <uint32_t *> group.data
        cdef int m = 0 if mode is None else mode
        cdef uint64_t db = <uint64_t> draw_base
        cdef float total = 0
        cdef int rc
        with nogil:
            rc = dist_gibbs_predict(self.ptr, rows, ptrs, <float *> logp.data,
                                    gp, m, seed_state, db, &total)
        free(ptrs)
        check(rc)
        return logp, (None if mode is None else group), total

    def feature_candidates(self, int target, candidates):
        """The candidate words of predict_feature for `target`: the list
        given, or for None the whole domain (DD 0..dim-1, BB 0, 1, DPD
        0..dim-1 then OTHER).  -> uint32 array"""
        cdef SharedParams s
        if target < 0 or target >= len(self.shareds):
            raise RuntimeError("predict_feature: no such target feature")
        s = self.shareds[target]
        if candidates is not None:
            return value_words(s.c.kind, candidates).ravel()
        if s.c.kind == DIST_DD:
            return np.arange(s.c.dim, dtype=np.uint32)
        if s.c.kind == DIST_BB:
            return np.arange(2, dtype=np.uint32)
        if s.c.kind == DIST_DPD:
            return np.append(np.arange(s.c.dim, dtype=np.uint32),
                             np.uint32(0xFFFFFFFF))
        raise RuntimeError("predict_feature: this target needs a candidate "
                           "list")

    def predict_feature_dev(self, value_ptrs, size_t n_rows,
                            size_t observed_ptr, int target, candidates,
                            size_t joint_ptr, size_t base_ptr,
                            size_t choice_ptr, int mode, uint32_t seed_state,
                            draw_base=0, unsigned flags=0):
        """One feature's predictive given the others
        (dist_gibbs_predict_feature_dev): value_ptrs are device addresses of
        one column of n_rows words per feature (0 for the target's is fine),
        observed_ptr the device address of the rows' masks or 0, candidates a
        host list or None (the whole domain), joint_ptr [n_rows, C] / base_ptr
        / choice_ptr device addresses or 0."""
        cdef int n = len(self.shareds)
        if len(value_ptrs) != n:
            raise RuntimeError("one value column per feature")
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] cand = np.ascontiguousarray(
            self.feature_candidates(target, candidates), dtype=np.uint32)
        cdef size_t n_cand = cand.shape[0]
        cdef const uint32_t * cand_p = (
            NULL if candidates is None else <const uint32_t *> cand.data)
        cdef const uint32_t ** ptrs = <const uint32_t **> malloc(
            sizeof(void *) * (n + 1))
        cdef int i
        cdef size_t addr
        for i in range(n):
            addr = value_ptrs[i]
            ptrs[i] = <const uint32_t *> addr
        cdef uint64_t db = <uint64_t> draw_base
        cdef int rc
        with nogil:
            rc = dist_gibbs_predict_feature_dev(
                self.ptr, n_rows, ptrs, <const uint32_t *> observed_ptr,
                target, cand_p, n_cand, <float *> joint_ptr,
                <float *> base_ptr, <uint32_t *> choice_ptr, mode, seed_state,
                db, flags)
        free(ptrs)
        check(rc)

    def predict_feature(self, values, int target, candidates, observed, mode,
                        uint32_t seed_state, draw_base=0, unsigned flags=0):
        """One feature's predictive given the others, from host arrays
        (dist_gibbs_predict_feature): values is one array per feature (None
        for the target's is fine), candidates a list or None (the whole
        domain), observed one uint32 mask per row or None, mode 0 draws, 1
        takes the first maximum, None leaves the choice out.
        -> (joint [n, C], base [n], choice [n] or None)"""
        cdef int n = len(self.shareds)
        if len(values) != n:
            raise RuntimeError("one value column per feature")
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] cand = np.ascontiguousarray(
            self.feature_candidates(target, candidates), dtype=np.uint32)
        cdef size_t n_cand = cand.shape[0]
        cdef const uint32_t * cand_p = (
            NULL if candidates is None else <const uint32_t *> cand.data)
        cdef const uint32_t ** ptrs = <const uint32_t **> malloc(
            sizeof(void *) * (n + 1))
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] w
        cdef SharedParams s
        words = []
        cdef int i
        cdef Py_ssize_t rows = -1
        for i in range(n):
            if values[i] is None and i == target:
                ptrs[i] = NULL
                continue
            s = self.shareds[i]
            w = value_words(s.c.kind, values[i])
            if rows >= 0 and w.shape[0] != rows:
                free(ptrs)
                raise RuntimeError("feature columns differ in length")
            rows = w.shape[0]
            words.append(w)
            ptrs[i] = <const uint32_t *> w.data
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] mask
        cdef const uint32_t * mask_p = NULL
        if observed is not None:
            mask = np.ascontiguousarray(observed, dtype=np.uint32)
            if rows >= 0 and mask.shape[0] != rows:
                free(ptrs)
                raise RuntimeError("one mask per row")
            rows = mask.shape[0]
            mask_p = <const uint32_t *> mask.data
        if rows < 0:
            free(ptrs)
            raise RuntimeError("predict_feature: no column tells the number "
                               "of rows")
        cdef size_t n_rows = rows
        cdef cnp.ndarray[cnp.float32_t, ndim=2] joint = np.zeros(
            (rows, n_cand), np.float32)
        cdef cnp.ndarray[cnp.float32_t, ndim=1] base = np.zeros(
            rows, np.float32)
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] choice = np.zeros(
            rows, np.uint32)
        cdef uint32_t * cp = NULL if mode is None else <uint32_t *> choice.data
        cdef int m = 0 if mode is None else mode
        cdef uint64_t db = <uint64_t> draw_base
        cdef int rc
        with nogil:
            rc = dist_gibbs_predict_feature(
                self.ptr, n_rows, ptrs, mask_p, target, cand_p, n_cand,
                <float *> joint.data, <float *> base.data, cp, m, seed_state,
                db, flags)
        free(ptrs)
        check(rc)
        return joint, base, (None if mode is None else choice)

    def sample_rows_dev(self, value_ptrs, size_t n_rows, size_t observed_ptr,
                        out_ptrs, size_t group_ptr, uint32_t seed_state,
                        draw_base=0):
        """Whole rows and missing cells drawn from the mixture
        (dist_gibbs_sample_rows_dev): value_ptrs is None or one device
        address per feature (0 for a feature no row observes), observed_ptr
        the device address of the rows' masks or 0 (nothing observed),
        out_ptrs one device address per feature (may equal the value's),
        group_ptr a device address or 0."""
        cdef int n = len(self.shareds)
        if len(out_ptrs) != n or (value_ptrs is not None
                                  and len(value_ptrs) != n):
            raise RuntimeError("one column per feature")
        cdef const uint32_t ** ptrs = <const uint32_t **> malloc(
            sizeof(void *) * (n + 1))
        cdef uint32_t ** outs = <uint32_t **> malloc(sizeof(void *) * (n + 1))
        cdef int i
        cdef size_t addr
        for i in range(n):
            addr = 0 if value_ptrs is None else value_ptrs[i]
            ptrs[i] = <const uint32_t *> addr
            addr = out_ptrs[i]
            outs[i] = <uint32_t *> addr
        cdef uint64_t db = <uint64_t> draw_base
        cdef int rc
        cdef bint no_values = value_ptrs is None
        with nogil:
            rc = dist_gibbs_sample_rows_dev(
                self.ptr, n_rows, NULL if no_values else ptrs,
                <const uint32_t *> observed_ptr, outs,
                <uint32_t *> group_ptr, seed_state, db)
        free(ptrs)
        free(outs)
        check(rc)

    def sample_rows(self, n_rows, values, observed, uint32_t seed_state,
                    draw_base=0):
        """Whole rows and missing cells drawn from the mixture, from host
        arrays (dist_gibbs_sample_rows): values is None or one array per
        feature (None for a feature no row observes), observed one uint32
        mask per row (required with values) or None: nothing observed, n_rows
        rows.  -> (columns, groups): one completed array per feature
        (float32 for NormalInverseChiSq, uint32 otherwise) and the drawn
        groups as global ids"""
        cdef int n = len(self.shareds)
        if values is not None and len(values) != n:
            raise RuntimeError("one value column per feature")
        if values is not None and observed is None:
            raise RuntimeError("sample_rows: values need an observed mask")
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] mask
        cdef const uint32_t * mask_p = NULL
        cdef size_t rows
        if observed is not None:
            mask = np.ascontiguousarray(observed, dtype=np.uint32)
            rows = mask.shape[0]
            mask_p = <const uint32_t *> mask.data
        else:
            if n_rows is None:
                raise RuntimeError("sample_rows: neither n nor a mask tells "
                                   "the number of rows")
            rows = n_rows
        if n_rows is not None and <size_t> n_rows != rows:
            raise RuntimeError("one mask per row")
        cdef const uint32_t ** ptrs = <const uint32_t **> malloc(
            sizeof(void *) * (n + 1))
        cdef uint32_t ** outs = <uint32_t **> malloc(sizeof(void *) * (n + 1))
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] w
        cdef SharedParams s
        words = []
        outw = []
        cdef int i
        for i in range(n):
            ptrs[i] = NULL
            if values is not None and values[i] is not None:
                s = self.shareds[i]
                w = value_words(s.c.kind, values[i])
                if <size_t> w.shape[0] != rows:
                    free(ptrs)
                    free(outs)
                    raise RuntimeError("feature columns differ in length")
                words.append(w)
                ptrs[i] = <const uint32_t *> w.data
            w = np.zeros(max(rows, 1), np.uint32)
            outw.append(w)
            outs[i] = <uint32_t *> w.data
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] group = np.zeros(
            max(rows, 1), np.uint32)
        cdef uint64_t db = <uint64_t> draw_base
        cdef bint no_values = values is None
        cdef int rc
        with nogil:
            rc = dist_gibbs_sample_rows(
                self.ptr, rows, NULL if no_values else ptrs, mask_p, outs,
                <uint32_t *> group.data, seed_state, db)
        free(ptrs)
        free(outs)
        check(rc)
        cols = []
        for i in range(n):
            s = self.shareds[i]
            w = outw[i][:rows]
            cols.append(w.view(np.float32) if s.c.kind == DIST_NICH else w)
        return cols, group[:rows]

    def group_count(self):
        return checked_size(dist_gibbs_group_count(self.ptr))

    def row_count(self):
        return dist_gibbs_row_count(self.ptr)

    def counts(self):
        cdef cnp.ndarray[cnp.int32_t, ndim=1] out = np.zeros(
            self.group_count(), np.int32)
        check(dist_gibbs_counts(self.ptr, <int *> out.data))
        return out

    def assignments(self):
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] out = np.zeros(
            max(1, self.row_count()), np.uint32)
        check(dist_gibbs_assignments(self.ptr, <uint32_t *> out.data))
        return out[:self.row_count()]

    def get_group(self, int feature, size_t groupid):
        cdef SharedParams s = self.shareds[feature]
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] g = np.zeros(s.group_words(),
                                                            np.uint32)
        check(dist_gibbs_get_group(self.ptr, feature, groupid,
                                   <uint32_t *> g.data))
        return g

    def packed_to_global(self, uint32_t packed):
        cdef uint32_t out = 0
        check(dist_gibbs_packed_to_global(self.ptr, packed, &out))
        return out

    def global_to_packed(self, uint32_t global_):
        cdef uint32_t out = 0
        check(dist_gibbs_global_to_packed(self.ptr, global_, &out))
        return out

    def global_size(self):
        return checked_size(dist_gibbs_global_size(self.ptr))

    def sharded_device_normalise_ok(self, size_t n_batches, size_t batch_rows):
        cdef int ok = 0
        check(dist_gibbs_sharded_device_normalise_ok(self.ptr, n_batches,
                                                     batch_rows, &ok))
        return bool(ok)

    def validate(self, raise_on_failure=True):
        """dist_gibbs_validate: the statistics against a recount from the rows
        (mixture.hpp:152-163,440-444).  Returns the report as a dict; raises
        RuntimeError on an inconsistency unless raise_on_failure is False."""
        cdef dist_validate_report_t rep
        cdef int rc = dist_gibbs_validate(self.ptr, &rep)
        if rc == 1 or (rc and raise_on_failure):
            check(rc)
        return {"code": rep.code, "feature": rep.feature, "group": rep.group,
                "detail": rep.detail, "expected": rep.expected,
                "found": rep.found, "rows_assigned": rep.rows_assigned,
                "what": (<bytes> rep.what).decode()}

    def debug_counts(self):
        """dict of the engine's path diagnostics (dist_gibbs_debug_counts)"""
        cdef uint64_t out[21]
        check(dist_gibbs_debug_counts(self.ptr, out, 21))
        return {"value_sorted_batches": out[0], "other_batches": out[1],
                "band_launches": out[2], "running_sum_launches": out[3],
                "band_values_last": out[4], "handed_over_last": out[5],
                "stream_batches": out[6], "device_normalised": out[7],
                "narrow_batches": out[8], "scratch_batches": out[9],
                "fold_batches": out[10], "scan_batches": out[11],
                "merged_batches": out[12], "fused_batches": out[13],
                "resumed_runs": out[14], "chain_launches": out[15],
                "rows_folded_last": out[16], "rows_instance_last": out[17],
                "search_batches": out[18], "rows_certified": out[19],
                "rows_left_over": out[20]}

    def chain_launches(self):
        """launches of the exact-chain kernel this engine issued"""
        return self.debug_counts()["chain_launches"]

    def set_option(self, name, int value):
        check(dist_gibbs_set_option(self.ptr, name.encode(), value))

    def set_certified_search(self, int mode, int slack=0):
        """k_vs_search in k_vs_sample's place: 0 never, 1 auto, 2 wherever it
        applies; the certificate's bound times 2^slack (tests)"""
        check(dist_gibbs_set_certified_search(self.ptr, mode, slack))

    def path_counts(self):
        """-> (batches served by the value-sorted kernel, by the generic one)"""
        cdef uint64_t a = 0, b = 0
        check(dist_gibbs_path_counts(self.ptr, &a, &b))
        return a, b

    def float_delta_words(self):
        """doubles per image of the merged float statistics (0: the ordered
        replay is in use)"""
        return checked_size(dist_gibbs_float_delta_words(self.ptr))

    def batch_float_delta_dev(self, size_t ptr):
        check(dist_gibbs_batch_float_delta_dev(self.ptr, <double *> ptr))

    def batch_apply_float_delta_dev(self, size_t ptr):
        check(dist_gibbs_batch_apply_float_delta_dev(self.ptr,
                                                     <const double *> ptr))

    def export_float_moments_dev(self, size_t ptr):
        check(dist_gibbs_export_float_moments_dev(self.ptr, <double *> ptr))

    def import_float_moments_dev(self, size_t ptr):
        check(dist_gibbs_import_float_moments_dev(self.ptr,
                                                  <const double *> ptr))

    def phase_stats(self, reset=False):
        """-> ([ms of tables, score+sample, handed-over rows, statistics,
        group set + caches], sub-sweeps timed) with option phase_timing"""
        cdef double ms[5]
        cdef uint64_t n = 0
        check(dist_gibbs_phase_stats(self.ptr, ms, &n, 1 if reset else 0))
        return [ms[i] for i in range(5)], n

    def comm_stats(self, reset=False):
        """-> (ms, count) of the timed all-reduces of sweep_sharded"""
        cdef double ms = 0
        cdef uint64_t launches = 0
        check(dist_gibbs_comm_stats(self.ptr, &ms, &launches,
                                    1 if reset else 0))
        return ms, launches

    def kernel_stats(self, reset=False):
        """-> (ms, launches, rows) of the score+sample kernel (HIP events)"""
        cdef double ms = 0
        cdef uint64_t launches = 0, rows = 0
        check(dist_gibbs_kernel_stats(self.ptr, &ms, &launches, &rows,
                                      1 if reset else 0))
        return ms, launches, rows

    # -- hyper-parameters (include/distributions_hip.h, "engine
    # hyper-parameters") ------------------------------------------------------
    def shared(self, int feature):
        """-> SharedParams the engine currently runs feature `feature` under"""
        cdef SharedParams given, out = SharedParams()
        cdef cnp.ndarray[cnp.float32_t, ndim=1] b
        if not 0 <= feature < len(self.shareds):
            raise RuntimeError("ERROR shared: bad feature index")
        given = self.shareds[feature]
        if given.c.kind == DIST_DPD:
            b = np.zeros(given.c.dim, np.float32)
            out._betas = b
            out.c.betas = <const float *> b.data
        check(dist_gibbs_shared(self.ptr, feature, &out.c))
        return out

    def clustering(self):
        """-> PitmanYor's (alpha, d)"""
        cdef float alpha = 0, d = 0
        check(dist_gibbs_clustering(self.ptr, &alpha, &d))
        return alpha, d

    def score_data(self):
        """-> (float32 score_data per feature, score_counts of the clustering
        model)"""
        cdef cnp.ndarray[cnp.float32_t, ndim=1] out = np.zeros(
            len(self.shareds) + 1, np.float32)
        cdef float clustering = 0
        check(dist_gibbs_score_data(self.ptr, <float *> out.data, &clustering))
        return out[:len(self.shareds)].copy(), clustering

    cdef dist_shared_t * _candidates(self, shareds) except NULL:
        cdef size_t n = len(shareds)
        cdef dist_shared_t * arr = <dist_shared_t *> malloc(
            (n + 1) * sizeof(dist_shared_t))
        cdef SharedParams s
        cdef size_t i
        try:
            for i in range(n):
                s = shareds[i]
                arr[i] = s.c
        except:
            free(arr)
            raise
        return arr

    def score_data_grid(self, int feature, shareds):
        """shareds: SharedParams candidates for `feature` -> float32 scores"""
        cdef size_t n = len(shareds)
        cdef cnp.ndarray[cnp.float32_t, ndim=1] out = np.zeros(n, np.float32)
        cdef dist_shared_t * arr = self._candidates(shareds)
        cdef int rc
        with nogil:
            rc = dist_gibbs_score_data_grid(self.ptr, feature, arr, n,
                                            <float *> out.data)
        free(arr)
        check(rc)
        return out

    def score_counts_grid(self, alphas, ds):
        """-> float32 PitmanYor score_counts per (alphas[c], ds[c])"""
        cdef cnp.ndarray[cnp.float32_t, ndim=1] a = np.ascontiguousarray(
            alphas, dtype=np.float32)
        cdef cnp.ndarray[cnp.float32_t, ndim=1] d = np.ascontiguousarray(
            ds, dtype=np.float32)
        if a.shape[0] != d.shape[0]:
            raise ValueError("one d per alpha")
        cdef cnp.ndarray[cnp.float32_t, ndim=1] out = np.zeros(a.shape[0],
                                                               np.float32)
        check(dist_gibbs_score_counts_grid(
            self.ptr, <const float *> a.data, <const float *> d.data,
            a.shape[0], <float *> out.data))
        return out

    def set_shared(self, int feature, SharedParams shared):
        check(dist_gibbs_set_shared(self.ptr, feature, &shared.c))
        self.shareds[feature] = shared

    def set_clustering(self, float alpha, float d):
        check(dist_gibbs_set_clustering(self.ptr, alpha, d))

    def sample_hypers(self, int feature, shareds, uint32_t rng_state):
        """grid + draw + install on the device -> (index, new rng state)"""
        cdef size_t n = len(shareds), chosen = 0
        cdef dist_shared_t * arr = self._candidates(shareds)
        cdef int rc
        with nogil:
            rc = dist_gibbs_sample_hypers(self.ptr, feature, arr, n,
                                          &rng_state, &chosen)
        free(arr)
        check(rc)
        self.shareds[feature] = shareds[chosen]
        return chosen, rng_state

    def sample_clustering(self, alphas, ds, uint32_t rng_state):
        """-> (index, new rng state); (alphas[index], ds[index]) installed"""
        cdef cnp.ndarray[cnp.float32_t, ndim=1] a = np.ascontiguousarray(
            alphas, dtype=np.float32)
        cdef cnp.ndarray[cnp.float32_t, ndim=1] d = np.ascontiguousarray(
            ds, dtype=np.float32)
        if a.shape[0] != d.shape[0]:
            raise ValueError("one d per alpha")
        cdef size_t chosen = 0
        check(dist_gibbs_sample_clustering(
            self.ptr, <const float *> a.data, <const float *> d.data,
            a.shape[0], &rng_state, &chosen))
        return chosen, rng_state

    def sample_hypers_pass(self, int feature, grids, uint32_t rng_state,
                           coords=None):
        """a whole coordinate pass of a DirichletDiscrete feature
        (dist_gibbs_sample_hypers_pass): grids float32 [n_coords, G] or one
        row [G] for every step, coords default 0 .. dim-1
        -> (indices uint32 [n_coords], new rng state)"""
        cdef cnp.ndarray[cnp.int32_t, ndim=1] co
        cdef cnp.ndarray[cnp.float32_t, ndim=2] gr
        cdef size_t stride
        co, gr, stride = _pass_arguments(self, feature, grids, coords)
        cdef size_t n = co.shape[0], G = gr.shape[1]
        cdef cnp.ndarray[cnp.uint32_t, ndim=1] chosen = np.zeros(n, np.uint32)
        cdef int rc
        with nogil:
            rc = dist_gibbs_sample_hypers_pass(
                self.ptr, feature, <const int *> co.data, n,
                <const float *> gr.data, G, stride, &rng_state,
                <uint32_t *> chosen.data)
        check(rc)
        self.shareds[feature] = self.shared(feature)
        return chosen, rng_state

    def hyper_stats(self):
        """-> (accumulator chains, candidates scored, launches, calls)"""
        cdef uint64_t out[4]
        check(dist_gibbs_hyper_stats(self.ptr, out))
        return out[0], out[1], out[2], out[3]


def _pass_arguments(GibbsEngine first, int feature, grids, coords):
    """-> (coords int32 [n], grid float32 [n or 1, G], grid_stride)"""
    gr = np.ascontiguousarray(grids, dtype=np.float32)
    if gr.ndim not in (1, 2):
        raise ValueError("grids: [n_coords, G], or [G] for every step")
    if coords is None:
        coords = np.arange(first.shared(feature).dim)
    co = np.ascontiguousarray(coords, dtype=np.int32).ravel()
    if gr.ndim == 2 and gr.shape[0] != co.shape[0]:
        raise ValueError("one grid per coordinate step")
    stride = gr.shape[1] if gr.ndim == 2 else 0
    # (no negative index: the module is compiled with wraparound=False)
    if gr.ndim == 1:
        gr = gr.reshape(1, gr.shape[0])
    return co, gr, stride


def sample_hypers_pass_many(engines, int feature, grids, rng_states,
                            coords=None):
    """the pass on M engines in the same launches
    (dist_gibbs_sample_hypers_pass_many): engines = GibbsEngine objects
    -> (indices uint32 [M, n_coords], new states uint32 [M])"""
    cdef size_t m = len(engines)
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] st = np.ascontiguousarray(
        rng_states, dtype=np.uint32).copy()
    if <size_t> st.shape[0] != m:
        raise ValueError("one rng state per engine")
    cdef cnp.ndarray[cnp.int32_t, ndim=1] co
    cdef cnp.ndarray[cnp.float32_t, ndim=2] gr
    cdef size_t stride
    if not m:
        return np.zeros((0, 0), np.uint32), st
    co, gr, stride = _pass_arguments(engines[0], feature, grids, coords)
    cdef size_t n = co.shape[0], G = gr.shape[1]
    cdef cnp.ndarray[cnp.uint32_t, ndim=2] chosen = np.zeros((m, n),
                                                             np.uint32)
    cdef dist_gibbs_t ** ptrs = _engine_ptrs(engines)
    cdef int rc
    with nogil:
        rc = dist_gibbs_sample_hypers_pass_many(
            <dist_gibbs_t * const *> ptrs, m, feature,
            <const int *> co.data, n, <const float *> gr.data, G, stride,
            <uint32_t *> st.data, <uint32_t *> chosen.data)
    free(ptrs)
    check(rc)
    cdef GibbsEngine e
    for e in engines:
        e.shareds[feature] = e.shared(feature)
    return chosen, st


def sweep_sequential_many(engines, size_t row_begin, size_t row_end,
                          rng_states):
    """M independent exact chains in one launch (dist_gibbs_sweep_sequential_
    many): engines = GibbsEngine objects, rng_states = their engine states.
    -> the new states (numpy uint32)."""
    cdef size_t m = len(engines)
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] st = np.ascontiguousarray(
        rng_states, dtype=np.uint32).copy()
    if <size_t> st.shape[0] != m:
        raise ValueError("one rng state per engine")
    cdef dist_gibbs_t ** ptrs = <dist_gibbs_t **> malloc(
        (m if m else 1) * sizeof(dist_gibbs_t *))
    cdef size_t i
    cdef int rc
    cdef GibbsEngine e
    try:
        for i in range(m):
            e = engines[i]
            ptrs[i] = e.ptr
        with nogil:
            rc = dist_gibbs_sweep_sequential_many(
                <dist_gibbs_t * const *> ptrs, m, row_begin, row_end,
                <uint32_t *> st.data)
    finally:
        free(ptrs)
    check(rc)
    return st


cdef dist_gibbs_t ** _engine_ptrs(engines) except NULL:
    """a malloc'ed array of the engines' handles (None: a null handle)"""
    cdef size_t m = len(engines)
    cdef dist_gibbs_t ** ptrs = <dist_gibbs_t **> malloc(
        (m if m else 1) * sizeof(dist_gibbs_t *))
    cdef size_t i
    cdef GibbsEngine e
    for i in range(m):
        if engines[i] is None:
            ptrs[i] = NULL
            continue
        try:
            e = engines[i]
        except TypeError:
            free(ptrs)
            raise
        ptrs[i] = e.ptr
    return ptrs


def predict_many_dev(engines, value_ptrs, size_t n_rows, size_t logp_ptr,
                     size_t member_ptr, size_t group_ptr, int mode,
                     uint32_t seed_state, uint32_t member_seed_state,
                     draw_base=0, size_t members_logp_ptr=0,
                     size_t members_ld=0, bint prior_totals=True,
                     unsigned flags=0):
    """Held-out rows against M engines (dist_gibbs_predict_many_dev):
    engines = GibbsEngine objects, value_ptrs device addresses of one column
    of n_rows words per feature, the other pointers device addresses or 0.
    -> the engines' prior totals (numpy float32), or None"""
    cdef size_t m = len(engines)
    cdef size_t nf = len(value_ptrs)
    cdef const uint32_t ** cols = <const uint32_t **> malloc(
        sizeof(void *) * (nf + 1))
    cdef size_t i
    cdef size_t addr
    for i in range(nf):
        addr = value_ptrs[i]
        cols[i] = <const uint32_t *> addr
    cdef cnp.ndarray[cnp.float32_t, ndim=1] totals = np.zeros(
        m if m else 1, np.float32)
    cdef float * tp = <float *> totals.data if prior_totals else NULL
    cdef uint64_t db = <uint64_t> draw_base
    cdef dist_gibbs_t ** ptrs
    cdef int rc
    try:
        ptrs = _engine_ptrs(engines)
    except Exception:
        free(cols)
        raise
    with nogil:
        rc = dist_gibbs_predict_many_dev(
            <dist_gibbs_t * const *> ptrs, m, n_rows, cols,
            <float *> logp_ptr, <uint32_t *> member_ptr,
            <uint32_t *> group_ptr, mode, seed_state, member_seed_state, db,
            <float *> members_logp_ptr, members_ld, tp, flags)
    free(ptrs)
    free(cols)
    check(rc)
    return totals[:m].copy() if prior_totals else None


def predict_many(engines, values, mode, uint32_t seed_state,
                 uint32_t member_seed_state, draw_base=0, bint members=False,
                 unsigned flags=0):
    """Held-out rows against M engines from host arrays
    (dist_gibbs_predict_many): values is one array per feature; mode 0 draws,
    1 takes the first maximum, None leaves members and groups out.
    -> (logp, members or None, groups or None, members_logp [M, n] or None,
    prior_totals [M])"""
    cdef size_t m = len(engines)
    if m == 0 or engines[0] is None:
        raise RuntimeError("predict_many: no engine" if m == 0
                           else "null engine")
    cdef GibbsEngine first = engines[0]
    cdef int n = len(first.shareds)
    if len(values) != n:
        raise RuntimeError("one value column per feature")
    cdef const uint32_t ** cols = <const uint32_t **> malloc(
        sizeof(void *) * (n + 1))
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] w
    cdef SharedParams s
    words = []
    cdef int i
    cdef size_t rows = 0
    for i in range(n):
        s = first.shareds[i]
        w = value_words(s.c.kind, values[i])
        if i and <size_t> w.shape[0] != rows:
            free(cols)
            raise RuntimeError("feature columns differ in length")
        rows = w.shape[0]
        words.append(w)
        cols[i] = <const uint32_t *> w.data
    cdef cnp.ndarray[cnp.float32_t, ndim=1] logp = np.zeros(rows, np.float32)
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] member = np.zeros(rows, np.uint32)
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] group = np.zeros(rows, np.uint32)
    cdef cnp.ndarray[cnp.float32_t, ndim=2] planes = np.zeros(
        (m if members else 1, rows if members else 1), np.float32)
    cdef cnp.ndarray[cnp.float32_t, ndim=1] totals = np.zeros(m, np.float32)
    cdef uint32_t * mp = NULL if mode is None else <uint32_t *> member.data
    cdef uint32_t * gp = NULL if mode is None else <uint32_t *> group.data
    cdef float * pp = <float *> planes.data if members else NULL
    cdef int md = 0 if mode is None else mode
    cdef uint64_t db = <uint64_t> draw_base
    cdef dist_gibbs_t ** ptrs
    cdef int rc
    try:
        ptrs = _engine_ptrs(engines)
    except Exception:
        free(cols)
        raise
    with nogil:
        rc = dist_gibbs_predict_many(
            <dist_gibbs_t * const *> ptrs, m, rows, cols,
            <float *> logp.data, mp, gp, md, seed_state, member_seed_state,
            db, pp, rows, <float *> totals.data, flags)
    free(ptrs)
    free(cols)
    check(rc)
    return (logp, None if mode is None else member,
            None if mode is None else group, planes if members else None,
            totals)


cdef const uint32_t ** _address_columns(value_ptrs) except NULL:
    """a malloc'ed array of device addresses (one column per feature)"""
    cdef size_t nf = len(value_ptrs)
    cdef const uint32_t ** cols = <const uint32_t **> malloc(
        sizeof(void *) * (nf + 1))
    cdef size_t i
    cdef size_t addr
    for i in range(nf):
        try:
            addr = value_ptrs[i]
        except Exception:
            free(cols)
            raise
        cols[i] = <const uint32_t *> addr
    return cols


def _word_columns(GibbsEngine first, values):
    """values as one contiguous uint32 array per feature of `first`
    -> (arrays, rows)"""
    cdef int n = len(first.shareds)
    if len(values) != n:
        raise RuntimeError("one value column per feature")
    cdef SharedParams s
    cdef int i
    words = []
    rows = 0
    for i in range(n):
        s = first.shareds[i]
        w = value_words(s.c.kind, values[i])
        if i and w.shape[0] != rows:
            raise RuntimeError("feature columns differ in length")
        rows = w.shape[0]
        words.append(w)
    return words, rows


def coassign_many_dev(engines, q_ptrs, size_t n_q, t_ptrs, size_t n_t,
                      size_t out_ptr, size_t ld, bint single=False):
    """Co-assignment of row pairs over M engines
    (dist_gibbs_coassign_many_dev; single: dist_gibbs_coassign_dev on the one
    engine): q_ptrs / t_ptrs device addresses of one column per feature
    (t_ptrs None: the targets are the queries), out_ptr the device address of
    [n_q, ld] floats."""
    cdef size_t m = len(engines)
    if single and m != 1:
        raise RuntimeError("coassign: one engine")
    if m == 0 or engines[0] is None:
        raise RuntimeError("coassign_many: no engine" if m == 0
                           else "null engine")
    cdef GibbsEngine first = engines[0]
    if len(q_ptrs) != len(first.shareds) or (
            t_ptrs is not None and len(t_ptrs) != len(first.shareds)):
        raise RuntimeError("one value column per feature")
    cdef const uint32_t ** qc = _address_columns(q_ptrs)
    cdef const uint32_t ** tc = NULL
    cdef dist_gibbs_t ** ptrs
    cdef int rc
    try:
        if t_ptrs is not None:
            tc = _address_columns(t_ptrs)
        ptrs = _engine_ptrs(engines)
    except Exception:
        free(qc)
        free(tc)
        raise
    with nogil:
        if single:
            rc = dist_gibbs_coassign_dev(ptrs[0], n_q, qc, n_t, tc,
                                         <float *> out_ptr, ld)
        else:
            rc = dist_gibbs_coassign_many_dev(
                <dist_gibbs_t * const *> ptrs, m, n_q, qc, n_t, tc,
                <float *> out_ptr, ld)
    free(ptrs)
    free(qc)
    free(tc)
    check(rc)


def coassign_many(engines, values, other=None, bint single=False):
    """Co-assignment of row pairs over M engines from host arrays
    (dist_gibbs_coassign_many; single: dist_gibbs_coassign): values and
    other are one array per feature; other None: the targets are the
    queries.  -> float32 [n_q, n_t]"""
    cdef size_t m = len(engines)
    if m == 0 or engines[0] is None:
        raise RuntimeError("coassign_many: no engine" if m == 0
                           else "null engine")
    if single and m != 1:
        raise RuntimeError("coassign: one engine")
    cdef GibbsEngine first = engines[0]
    qw, rows_q = _word_columns(first, values)
    tw, rows_t = (None, rows_q) if other is None else _word_columns(first,
                                                                    other)
    cdef size_t nf = len(qw)
    cdef size_t n_q = rows_q, n_t = rows_t
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] w
    cdef cnp.ndarray[cnp.float32_t, ndim=2] out = np.zeros((n_q, n_t),
                                                           np.float32)
    cdef const uint32_t ** qc = <const uint32_t **> malloc(
        sizeof(void *) * (nf + 1))
    cdef const uint32_t ** tc = NULL
    cdef size_t i
    for i in range(nf):
        w = qw[i]
        qc[i] = <const uint32_t *> w.data
    if tw is not None:
        tc = <const uint32_t **> malloc(sizeof(void *) * (nf + 1))
        for i in range(nf):
            w = tw[i]
            tc[i] = <const uint32_t *> w.data
    cdef dist_gibbs_t ** ptrs
    cdef int rc
    try:
        ptrs = _engine_ptrs(engines)
    except Exception:
        free(qc)
        free(tc)
        raise
    with nogil:
        if single:
            rc = dist_gibbs_coassign(ptrs[0], n_q, qc, n_t, tc,
                                     <float *> out.data, n_t)
        else:
            rc = dist_gibbs_coassign_many(
                <dist_gibbs_t * const *> ptrs, m, n_q, qc, n_t, tc,
                <float *> out.data, n_t)
    free(ptrs)
    free(qc)
    free(tc)
    check(rc)
    return out


def _label_columns(columns, bint dev, size_t n_rows):
    """-> (what keeps the columns alive, a malloc'ed array of their
    addresses): device addresses as they are, host columns as contiguous
    uint32 arrays of n_rows words"""
    cdef size_t p = len(columns)
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] w
    cdef size_t i
    if dev:
        return None, <size_t> _address_columns(columns)
    words = []
    for c in columns:
        w = np.ascontiguousarray(c, np.uint32).reshape(-1)
        if <size_t> w.shape[0] != n_rows:
            raise RuntimeError("partition_agreement: a label column of %d "
                               "rows, not %d" % (w.shape[0], n_rows))
        words.append(w)
    cdef const uint32_t ** cols = <const uint32_t **> malloc(
        sizeof(void *) * (p + 1))
    for i in range(p):
        w = words[i]
        cols[i] = <const uint32_t *> w.data
    return words, <size_t> cols


def partition_agreement_many(engines, size_t n_rows, columns, n_labels,
                             bint nlogn=True, bint dev=False,
                             bint single=False):
    """sq and nlogn of the partitions (the engines' resident assignments,
    then `columns`) of the same n_rows rows
    (dist_gibbs_partition_agreement_many[_dev]; single:
    dist_gibbs_partition_agreement; no engine: dist_partition_agreement[_dev]).
    columns: host uint32 arrays, or with dev their device addresses; n_labels
    one exclusive bound per column.
    -> (uint64 [P, P], float64 [P, P] or None)"""
    cdef size_t m = len(engines), x = len(columns)
    if single and m != 1:
        raise RuntimeError("partition_agreement: one engine")
    if len(n_labels) != x:
        raise RuntimeError("partition_agreement: one n_labels per column")
    cdef size_t p = m + x
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] bounds = np.ascontiguousarray(
        np.asarray(n_labels, np.uint32).reshape(-1))
    cdef cnp.ndarray[cnp.uint64_t, ndim=2] sq = np.zeros((p, p), np.uint64)
    cdef size_t pn = p if nlogn else 0
    cdef cnp.ndarray[cnp.float64_t, ndim=2] nl = np.zeros((pn, pn),
                                                          np.float64)
    keep, addr = _label_columns(columns, dev, n_rows)
    cdef const uint32_t ** cols = <const uint32_t **> <size_t> addr
    cdef dist_gibbs_t ** ptrs
    try:
        ptrs = _engine_ptrs(engines)
    except Exception:
        free(cols)
        raise
    cdef uint64_t * sq_p = <uint64_t *> sq.data
    cdef double * nl_p = NULL
    if nlogn:
        nl_p = <double *> nl.data
    cdef const uint32_t * nb = <const uint32_t *> bounds.data
    cdef int rc
    with nogil:
        if m == 0 and dev:
            rc = dist_partition_agreement_dev(n_rows, x, cols, nb, sq_p, nl_p)
        elif m == 0:
            rc = dist_partition_agreement(n_rows, x, cols, nb, sq_p, nl_p)
        elif dev:
            rc = dist_gibbs_partition_agreement_many_dev(
                <dist_gibbs_t * const *> ptrs, m, n_rows, cols, x, nb, sq_p,
                nl_p)
        elif single:
            rc = dist_gibbs_partition_agreement(ptrs[0], n_rows, cols, x, nb,
                                                sq_p, nl_p)
        else:
            rc = dist_gibbs_partition_agreement_many(
                <dist_gibbs_t * const *> ptrs, m, n_rows, cols, x, nb, sq_p,
                nl_p)
    free(ptrs)
    free(cols)
    check(rc)
    return sq, (nl if nlogn else None)


def coassign_resident_many_dev(engines, size_t rows_a_ptr, size_t na,
                               size_t rows_b_ptr, size_t nb, size_t out_ptr,
                               size_t ld, bint single=False):
    """Co-assignment of resident rows over M engines
    (dist_gibbs_coassign_resident_many_dev; single:
    dist_gibbs_coassign_resident_dev): device addresses of uint32 row indices
    (rows_b_ptr 0: the rows of rows_a) and of [na, ld] floats."""
    cdef size_t m = len(engines)
    if single and m != 1:
        raise RuntimeError("coassign_resident: one engine")
    cdef dist_gibbs_t ** ptrs = _engine_ptrs(engines)
    cdef int rc
    with nogil:
        if single:
            rc = dist_gibbs_coassign_resident_dev(
                ptrs[0], <const uint32_t *> rows_a_ptr, na,
                <const uint32_t *> rows_b_ptr, nb, <float *> out_ptr, ld)
        else:
            rc = dist_gibbs_coassign_resident_many_dev(
                <dist_gibbs_t * const *> ptrs, m,
                <const uint32_t *> rows_a_ptr, na,
                <const uint32_t *> rows_b_ptr, nb, <float *> out_ptr, ld)
    free(ptrs)
    check(rc)


def coassign_resident_many(engines, rows, other=None, bint single=False):
    """Co-assignment of resident rows over M engines from host index arrays
    (dist_gibbs_coassign_resident_many; single: dist_gibbs_coassign_resident);
    other None: the rows themselves.  -> float32 [len(rows), len(other)]"""
    cdef size_t m = len(engines)
    if single and m != 1:
        raise RuntimeError("coassign_resident: one engine")
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] ra = _row_indices(rows)
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] rb = (
        ra if other is None else _row_indices(other))
    cdef size_t na = ra.shape[0], nb = rb.shape[0]
    cdef cnp.ndarray[cnp.float32_t, ndim=2] out = np.zeros((na, nb),
                                                           np.float32)
    cdef const uint32_t * pa = <const uint32_t *> ra.data
    cdef const uint32_t * pb = (NULL if other is None
                                else <const uint32_t *> rb.data)
    cdef dist_gibbs_t ** ptrs = _engine_ptrs(engines)
    cdef int rc
    with nogil:
        if single:
            rc = dist_gibbs_coassign_resident(ptrs[0], pa, na, pb, nb,
                                              <float *> out.data, nb)
        else:
            rc = dist_gibbs_coassign_resident_many(
                <dist_gibbs_t * const *> ptrs, m, pa, na, pb, nb,
                <float *> out.data, nb)
    free(ptrs)
    check(rc)
    return out


def _row_indices(rows):
    """row indices as a contiguous uint32 array; one that does not fit 32
    bits is out of every engine's range"""
    a = np.asarray(rows).reshape(-1)
    if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
        raise RuntimeError("coassign_resident_many: row index outside the "
                           "engines' rows")
    return np.ascontiguousarray(a, np.uint32)


COASSIGN_EXCLUDE_SELF = 1


def coassign_topk_many_dev(engines, q_ptrs, size_t n_q, t_ptrs, size_t n_t,
                           size_t k, unsigned flags, size_t index_ptr,
                           size_t prob_ptr, size_t ld, bint single=False):
    """Per query the k most co-assigned targets over M engines
    (dist_gibbs_coassign_topk_many_dev; single: dist_gibbs_coassign_topk_dev
    on the one engine): q_ptrs / t_ptrs as coassign_many_dev's, index_ptr and
    prob_ptr the device addresses of [n_q, ld] uint32 words and floats."""
    cdef size_t m = len(engines)
    if single and m != 1:
        raise RuntimeError("coassign_topk: one engine")
    if m == 0 or engines[0] is None:
        raise RuntimeError("coassign_topk_many: no engine" if m == 0
                           else "null engine")
    cdef GibbsEngine first = engines[0]
    if len(q_ptrs) != len(first.shareds) or (
            t_ptrs is not None and len(t_ptrs) != len(first.shareds)):
        raise RuntimeError("one value column per feature")
    cdef const uint32_t ** qc = _address_columns(q_ptrs)
    cdef const uint32_t ** tc = NULL
    cdef dist_gibbs_t ** ptrs
    cdef int rc
    try:
        if t_ptrs is not None:
            tc = _address_columns(t_ptrs)
        ptrs = _engine_ptrs(engines)
    except Exception:
        free(qc)
        free(tc)
        raise
    with nogil:
        if single:
            rc = dist_gibbs_coassign_topk_dev(
                ptrs[0], n_q, qc, n_t, tc, k, flags, <uint32_t *> index_ptr,
                <float *> prob_ptr, ld)
        else:
            rc = dist_gibbs_coassign_topk_many_dev(
                <dist_gibbs_t * const *> ptrs, m, n_q, qc, n_t, tc, k, flags,
                <uint32_t *> index_ptr, <float *> prob_ptr, ld)
    free(ptrs)
    free(qc)
    free(tc)
    check(rc)


def coassign_topk_many(engines, values, other, size_t k, unsigned flags,
                       bint single=False, ld=None):
    """Per query the k most co-assigned targets over M engines from host
    arrays (dist_gibbs_coassign_topk_many; single: dist_gibbs_coassign_topk):
    values and other as coassign_many's; ld: the row stride handed to the
    library (None: k).  -> (uint32 [n_q, k], float32 [n_q, k])"""
    cdef size_t m = len(engines)
    if m == 0 or engines[0] is None:
        raise RuntimeError("coassign_topk_many: no engine" if m == 0
                           else "null engine")
    if single and m != 1:
        raise RuntimeError("coassign_topk: one engine")
    cdef GibbsEngine first = engines[0]
    qw, rows_q = _word_columns(first, values)
    tw, rows_t = (None, rows_q) if other is None else _word_columns(first,
                                                                    other)
    cdef size_t nf = len(qw)
    cdef size_t n_q = rows_q, n_t = rows_t
    cdef size_t stride = k if ld is None else ld
    # (a stride below k is the library's to refuse: room for k all the same)
    cdef size_t width = max(stride, k)
    cdef cnp.ndarray[cnp.uint32_t, ndim=2] index = np.zeros((n_q, width),
                                                            np.uint32)
    cdef cnp.ndarray[cnp.float32_t, ndim=2] prob = np.zeros((n_q, width),
                                                            np.float32)
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] w
    cdef const uint32_t ** qc = <const uint32_t **> malloc(
        sizeof(void *) * (nf + 1))
    cdef const uint32_t ** tc = NULL
    cdef size_t i
    for i in range(nf):
        w = qw[i]
        qc[i] = <const uint32_t *> w.data
    if tw is not None:
        tc = <const uint32_t **> malloc(sizeof(void *) * (nf + 1))
        for i in range(nf):
            w = tw[i]
            tc[i] = <const uint32_t *> w.data
    cdef dist_gibbs_t ** ptrs
    cdef int rc
    try:
        ptrs = _engine_ptrs(engines)
    except Exception:
        free(qc)
        free(tc)
        raise
    with nogil:
        if single:
            rc = dist_gibbs_coassign_topk(
                ptrs[0], n_q, qc, n_t, tc, k, flags,
                <uint32_t *> index.data, <float *> prob.data, stride)
        else:
            rc = dist_gibbs_coassign_topk_many(
                <dist_gibbs_t * const *> ptrs, m, n_q, qc, n_t, tc, k, flags,
                <uint32_t *> index.data, <float *> prob.data, stride)
    free(ptrs)
    free(qc)
    free(tc)
    check(rc)
    return (np.ascontiguousarray(index[:, :k]),
            np.ascontiguousarray(prob[:, :k]))


def search_resident_many_dev(engines, q_ptrs, size_t n_q, size_t row_begin,
                             size_t row_end, size_t k, unsigned flags,
                             size_t index_ptr, size_t prob_ptr, size_t ld,
                             bint single=False):
    """Per held-out query the k most co-assigned RESIDENT rows of [row_begin,
    row_end) over M engines (dist_gibbs_search_resident_many_dev; single:
    dist_gibbs_search_resident_dev): q_ptrs as coassign_many_dev's, index_ptr
    and prob_ptr the device addresses of [n_q, ld] uint32 words and floats."""
    cdef size_t m = len(engines)
    if single and m != 1:
        raise RuntimeError("search_resident: one engine")
    cdef GibbsEngine first
    if m and engines[0] is not None:
        first = engines[0]
        if len(q_ptrs) != len(first.shareds):
            raise RuntimeError("one value column per feature")
    cdef const uint32_t ** qc = _address_columns(q_ptrs)
    cdef dist_gibbs_t ** ptrs
    cdef int rc
    try:
        ptrs = _engine_ptrs(engines)
    except Exception:
        free(qc)
        raise
    with nogil:
        if single:
            rc = dist_gibbs_search_resident_dev(
                ptrs[0], n_q, qc, row_begin, row_end, k, flags,
                <uint32_t *> index_ptr, <float *> prob_ptr, ld)
        else:
            rc = dist_gibbs_search_resident_many_dev(
                <dist_gibbs_t * const *> ptrs, m, n_q, qc, row_begin, row_end,
                k, flags, <uint32_t *> index_ptr, <float *> prob_ptr, ld)
    free(ptrs)
    free(qc)
    check(rc)


def search_resident_many(engines, values, size_t row_begin, size_t row_end,
                         size_t k, unsigned flags=0, bint single=False,
                         ld=None):
    """search_resident_many_dev from host arrays
    (dist_gibbs_search_resident_many; single: dist_gibbs_search_resident);
    ld: the row stride handed to the library (None: k).
    -> (uint32 [n_q, k], float32 [n_q, k])"""
    cdef size_t m = len(engines)
    if single and m != 1:
        raise RuntimeError("search_resident: one engine")
    cdef GibbsEngine first
    qw, rows_q = [], 0
    if m and engines[0] is not None:
        first = engines[0]
        qw, rows_q = _word_columns(first, values)
    cdef size_t nf = len(qw)
    cdef size_t n_q = rows_q
    cdef size_t stride = k if ld is None else ld
    cdef size_t width = max(stride, k)
    cdef cnp.ndarray[cnp.uint32_t, ndim=2] index = np.zeros((n_q, width),
                                                            np.uint32)
    cdef cnp.ndarray[cnp.float32_t, ndim=2] prob = np.zeros((n_q, width),
                                                            np.float32)
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] w
    cdef const uint32_t ** qc = <const uint32_t **> malloc(
        sizeof(void *) * (nf + 1))
    cdef size_t i
    for i in range(nf):
        w = qw[i]
        qc[i] = <const uint32_t *> w.data
    cdef dist_gibbs_t ** ptrs
    cdef int rc
    try:
        ptrs = _engine_ptrs(engines)
    except Exception:
        free(qc)
        raise
    with nogil:
        if single:
            rc = dist_gibbs_search_resident(
                ptrs[0], n_q, qc, row_begin, row_end, k, flags,
                <uint32_t *> index.data, <float *> prob.data, stride)
        else:
            rc = dist_gibbs_search_resident_many(
                <dist_gibbs_t * const *> ptrs, m, n_q, qc, row_begin, row_end,
                k, flags, <uint32_t *> index.data, <float *> prob.data,
                stride)
    free(ptrs)
    free(qc)
    check(rc)
    return (np.ascontiguousarray(index[:, :k]),
            np.ascontiguousarray(prob[:, :k]))


def coassign_resident_topk_many_dev(engines, size_t rows_ptr, size_t n_q,
                                    size_t row_begin, size_t row_end,
                                    size_t k, unsigned flags,
                                    size_t index_ptr, size_t prob_ptr,
                                    size_t ld, bint single=False):
    """Per resident query row the k most co-assigned RESIDENT rows of
    [row_begin, row_end) over M engines
    (dist_gibbs_coassign_resident_topk_many_dev; single:
    dist_gibbs_coassign_resident_topk_dev): device addresses of uint32 row
    indices and of [n_q, ld] uint32 words and floats."""
    cdef size_t m = len(engines)
    if single and m != 1:
        raise RuntimeError("coassign_resident_topk: one engine")
    cdef dist_gibbs_t ** ptrs = _engine_ptrs(engines)
    cdef int rc
    with nogil:
        if single:
            rc = dist_gibbs_coassign_resident_topk_dev(
                ptrs[0], <const uint32_t *> rows_ptr, n_q, row_begin, row_end,
                k, flags, <uint32_t *> index_ptr, <float *> prob_ptr, ld)
        else:
            rc = dist_gibbs_coassign_resident_topk_many_dev(
                <dist_gibbs_t * const *> ptrs, m,
                <const uint32_t *> rows_ptr, n_q, row_begin, row_end, k,
                flags, <uint32_t *> index_ptr, <float *> prob_ptr, ld)
    free(ptrs)
    check(rc)


def coassign_resident_topk_many(engines, rows, size_t row_begin,
                                size_t row_end, size_t k, unsigned flags=0,
                                bint single=False, ld=None):
    """coassign_resident_topk_many_dev from a host index array
    (dist_gibbs_coassign_resident_topk_many; single:
    dist_gibbs_coassign_resident_topk) -> (uint32 [n_q, k], float32 [n_q, k])"""
    cdef size_t m = len(engines)
    if single and m != 1:
        raise RuntimeError("coassign_resident_topk: one engine")
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] ra = _row_indices(rows)
    cdef size_t n_q = ra.shape[0]
    cdef size_t stride = k if ld is None else ld
    cdef size_t width = max(stride, k)
    cdef cnp.ndarray[cnp.uint32_t, ndim=2] index = np.zeros((n_q, width),
                                                            np.uint32)
    cdef cnp.ndarray[cnp.float32_t, ndim=2] prob = np.zeros((n_q, width),
                                                            np.float32)
    cdef const uint32_t * pa = <const uint32_t *> ra.data
    cdef dist_gibbs_t ** ptrs = _engine_ptrs(engines)
    cdef int rc
    with nogil:
        if single:
            rc = dist_gibbs_coassign_resident_topk(
                ptrs[0], pa, n_q, row_begin, row_end, k, flags,
                <uint32_t *> index.data, <float *> prob.data, stride)
        else:
            rc = dist_gibbs_coassign_resident_topk_many(
                <dist_gibbs_t * const *> ptrs, m, pa, n_q, row_begin, row_end,
                k, flags, <uint32_t *> index.data, <float *> prob.data,
                stride)
    free(ptrs)
    check(rc)
    return (np.ascontiguousarray(index[:, :k]),
            np.ascontiguousarray(prob[:, :k]))


def responsibilities_dev(GibbsEngine engine, value_ptrs, size_t n_rows,
                         size_t resp_ptr, size_t ld):
    """One engine's group posterior of held-out rows
    (dist_gibbs_responsibilities_dev): resp_ptr the device address of
    [groups, ld] floats, k-major."""
    if len(value_ptrs) != len(engine.shareds):
        raise RuntimeError("one value column per feature")
    cdef const uint32_t ** cols = _address_columns(value_ptrs)
    cdef int rc
    with nogil:
        rc = dist_gibbs_responsibilities_dev(engine.ptr, n_rows, cols,
                                             <float *> resp_ptr, ld)
    free(cols)
    check(rc)


def responsibilities(GibbsEngine engine, values):
    """One engine's group posterior of held-out rows from host arrays
    (dist_gibbs_responsibilities) -> float32 [groups, n], k-major"""
    words, rows = _word_columns(engine, values)
    cdef size_t nf = len(words)
    cdef size_t n = rows
    cdef size_t groups = engine.group_count()
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] w
    cdef cnp.ndarray[cnp.float32_t, ndim=2] resp = np.zeros((groups, n),
                                                            np.float32)
    cdef const uint32_t ** cols = <const uint32_t **> malloc(
        sizeof(void *) * (nf + 1))
    cdef size_t i
    for i in range(nf):
        w = words[i]
        cols[i] = <const uint32_t *> w.data
    cdef int rc
    with nogil:
        rc = dist_gibbs_responsibilities(engine.ptr, n, cols,
                                         <float *> resp.data, n)
    free(cols)
    check(rc)
    return resp


def predict_feature_many_dev(engines, value_ptrs, size_t n_rows,
                             size_t observed_ptr, int target, candidates,
                             size_t joint_ptr, size_t base_ptr,
                             size_t choice_ptr, size_t member_ptr, int mode,
                             uint32_t seed_state, uint32_t member_seed_state,
                             draw_base=0, size_t members_joint_ptr=0,
                             size_t members_joint_ld=0,
                             size_t members_base_ptr=0,
                             size_t members_base_ld=0,
                             bint prior_totals=True, unsigned flags=0):
    """One feature's predictive averaged over M engines
    (dist_gibbs_predict_feature_many_dev): engines = GibbsEngine objects,
    value_ptrs device addresses of one column of n_rows words per feature (0
    for the target's is fine), observed_ptr the device address of the rows'
    masks or 0, candidates a host list or None (the whole domain), the other
    pointers device addresses or 0.
    -> the engines' prior totals (numpy float32), or None"""
    cdef size_t m = len(engines)
    if m == 0 or engines[0] is None:
        raise RuntimeError("predict_feature_many: no engine" if m == 0
                           else "null engine")
    cdef GibbsEngine first = engines[0]
    cdef size_t nf = len(value_ptrs)
    if nf != len(first.shareds):
        raise RuntimeError("one value column per feature")
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] cand = np.ascontiguousarray(
        first.feature_candidates(target, candidates), dtype=np.uint32)
    cdef size_t n_cand = cand.shape[0]
    cdef const uint32_t * cand_p = (
        NULL if candidates is None else <const uint32_t *> cand.data)
    cdef const uint32_t ** cols = <const uint32_t **> malloc(
        sizeof(void *) * (nf + 1))
    cdef size_t i
    cdef size_t addr
    for i in range(nf):
        addr = value_ptrs[i]
        cols[i] = <const uint32_t *> addr
    cdef cnp.ndarray[cnp.float32_t, ndim=1] totals = np.zeros(m, np.float32)
    cdef float * tp = <float *> totals.data if prior_totals else NULL
    cdef uint64_t db = <uint64_t> draw_base
    cdef dist_gibbs_t ** ptrs
    cdef int rc
    try:
        ptrs = _engine_ptrs(engines)
    except Exception:
        free(cols)
        raise
    with nogil:
        rc = dist_gibbs_predict_feature_many_dev(
            <dist_gibbs_t * const *> ptrs, m, n_rows, cols,
            <const uint32_t *> observed_ptr, target, cand_p, n_cand,
            <float *> joint_ptr, <float *> base_ptr, <uint32_t *> choice_ptr,
            <uint32_t *> member_ptr, mode, seed_state, member_seed_state, db,
            <float *> members_joint_ptr, members_joint_ld,
            <float *> members_base_ptr, members_base_ld, tp, flags)
    free(ptrs)
    free(cols)
    check(rc)
    return totals.copy() if prior_totals else None


def predict_feature_many(engines, values, int target, candidates, observed,
                         mode, uint32_t seed_state,
                         uint32_t member_seed_state, draw_base=0,
                         bint members=False, unsigned flags=0):
    """One feature's predictive averaged over M engines, from host arrays
    (dist_gibbs_predict_feature_many): values is one array per feature (None
    for the target's is fine), candidates a list or None (the whole domain),
    observed one uint32 mask per row or None; mode 0 draws, 1 takes the first
    maximum, None leaves choice and member out.
    -> (joint [n, C], base [n], choice or None, member or None,
    members_joint [M, n, C] or None, members_base [M, n] or None,
    prior_totals [M])"""
    cdef size_t m = len(engines)
    if m == 0 or engines[0] is None:
        raise RuntimeError("predict_feature_many: no engine" if m == 0
                           else "null engine")
    cdef GibbsEngine first = engines[0]
    cdef int n = len(first.shareds)
    if len(values) != n:
        raise RuntimeError("one value column per feature")
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] cand = np.ascontiguousarray(
        first.feature_candidates(target, candidates), dtype=np.uint32)
    cdef size_t n_cand = cand.shape[0]
    cdef const uint32_t * cand_p = (
        NULL if candidates is None else <const uint32_t *> cand.data)
    cdef const uint32_t ** cols = <const uint32_t **> malloc(
        sizeof(void *) * (n + 1))
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] w
    cdef SharedParams s
    words = []
    cdef int i
    cdef Py_ssize_t rows = -1
    for i in range(n):
        if values[i] is None and i == target:
            cols[i] = NULL
            continue
        s = first.shareds[i]
        w = value_words(s.c.kind, values[i])
        if rows >= 0 and w.shape[0] != rows:
            free(cols)
            raise RuntimeError("feature columns differ in length")
        rows = w.shape[0]
        words.append(w)
        cols[i] = <const uint32_t *> w.data
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] mask
    cdef const uint32_t * mask_p = NULL
    if observed is not None:
        mask = np.ascontiguousarray(observed, dtype=np.uint32)
        if rows >= 0 and mask.shape[0] != rows:
            free(cols)
            raise RuntimeError("one mask per row")
        rows = mask.shape[0]
        mask_p = <const uint32_t *> mask.data
    if rows < 0:
        free(cols)
        raise RuntimeError("predict_feature_many: no column tells the "
                           "number of rows")
    cdef size_t n_rows = rows
    cdef cnp.ndarray[cnp.float32_t, ndim=2] joint = np.zeros(
        (rows, n_cand), np.float32)
    cdef cnp.ndarray[cnp.float32_t, ndim=1] base = np.zeros(rows, np.float32)
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] choice = np.zeros(rows, np.uint32)
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] member = np.zeros(rows, np.uint32)
    cdef cnp.ndarray[cnp.float32_t, ndim=3] pj = np.zeros(
        (m if members else 1, rows if members else 1,
         n_cand if members else 1), np.float32)
    cdef cnp.ndarray[cnp.float32_t, ndim=2] pb = np.zeros(
        (m if members else 1, rows if members else 1), np.float32)
    cdef cnp.ndarray[cnp.float32_t, ndim=1] totals = np.zeros(m, np.float32)
    cdef uint32_t * cp = NULL if mode is None else <uint32_t *> choice.data
    cdef uint32_t * mp = NULL if mode is None else <uint32_t *> member.data
    cdef float * pjp = <float *> pj.data if members else NULL
    cdef float * pbp = <float *> pb.data if members else NULL
    cdef int md = 0 if mode is None else mode
    cdef uint64_t db = <uint64_t> draw_base
    cdef dist_gibbs_t ** ptrs
    cdef int rc
    try:
        ptrs = _engine_ptrs(engines)
    except Exception:
        free(cols)
        raise
    with nogil:
        rc = dist_gibbs_predict_feature_many(
            <dist_gibbs_t * const *> ptrs, m, n_rows, cols, mask_p, target,
            cand_p, n_cand, <float *> joint.data, <float *> base.data, cp,
            mp, md, seed_state, member_seed_state, db, pjp, n_rows * n_cand,
            pbp, n_rows, <float *> totals.data, flags)
    free(ptrs)
    free(cols)
    check(rc)
    return (joint, base, None if mode is None else choice,
            None if mode is None else member, pj if members else None,
            pb if members else None, totals)


def sample_rows_many_dev(engines, value_ptrs, size_t n_rows,
                         size_t observed_ptr, out_ptrs, size_t group_ptr,
                         size_t member_ptr, size_t base_ptr,
                         uint32_t seed_state, uint32_t member_seed_state,
                         draw_base=0, unsigned flags=0):
    """Whole rows and missing cells drawn from an ensemble of M engines
    (dist_gibbs_sample_rows_many_dev): engines = GibbsEngine objects,
    value_ptrs is None or one device address per feature (0 for a feature no
    row observes), observed_ptr the device address of the rows' masks or 0
    (nothing observed), out_ptrs one device address per feature (may equal the
    value's), group_ptr, member_ptr and base_ptr device addresses or 0."""
    cdef size_t m = len(engines)
    if m == 0 or engines[0] is None:
        raise RuntimeError("sample_rows_many: no engine" if m == 0
                           else "null engine")
    cdef GibbsEngine first = engines[0]
    cdef size_t nf = len(first.shareds)
    if len(out_ptrs) != nf or (value_ptrs is not None
                               and len(value_ptrs) != nf):
        raise RuntimeError("one column per feature")
    cdef const uint32_t ** cols = <const uint32_t **> malloc(
        sizeof(void *) * (nf + 1))
    cdef uint32_t ** outs = <uint32_t **> malloc(sizeof(void *) * (nf + 1))
    cdef size_t i
    cdef size_t addr
    for i in range(nf):
        addr = 0 if value_ptrs is None else value_ptrs[i]
        cols[i] = <const uint32_t *> addr
        addr = out_ptrs[i]
        outs[i] = <uint32_t *> addr
    cdef uint64_t db = <uint64_t> draw_base
    cdef bint no_values = value_ptrs is None
    cdef dist_gibbs_t ** ptrs
    cdef int rc
    try:
        ptrs = _engine_ptrs(engines)
    except Exception:
        free(cols)
        free(outs)
        raise
    with nogil:
        rc = dist_gibbs_sample_rows_many_dev(
            <dist_gibbs_t * const *> ptrs, m, n_rows,
            NULL if no_values else cols, <const uint32_t *> observed_ptr,
            outs, <uint32_t *> group_ptr, <uint32_t *> member_ptr,
            <float *> base_ptr, seed_state, member_seed_state, db, flags)
    free(ptrs)
    free(cols)
    free(outs)
    check(rc)


def sample_rows_many(engines, n_rows, values, observed, uint32_t seed_state,
                     uint32_t member_seed_state, draw_base=0,
                     unsigned flags=0):
    """Whole rows and missing cells drawn from an ensemble of M engines, from
    host arrays (dist_gibbs_sample_rows_many): values is None or one array per
    feature (None for a feature no row observes), observed one uint32 mask per
    row (required with values) or None: nothing observed, n_rows rows.
    -> (columns, groups, members, base): one completed array per feature
    (float32 for NormalInverseChiSq, uint32 otherwise), the drawn groups as
    global ids of the drawn members, the members, and the ensemble's log
    marginal of the observed cells"""
    cdef size_t m = len(engines)
    if m == 0 or engines[0] is None:
        raise RuntimeError("sample_rows_many: no engine" if m == 0
                           else "null engine")
    cdef GibbsEngine first = engines[0]
    cdef int n = len(first.shareds)
    if values is not None and len(values) != n:
        raise RuntimeError("one value column per feature")
    if values is not None and observed is None:
        raise RuntimeError("sample_rows_many: values need an observed mask")
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] mask
    cdef const uint32_t * mask_p = NULL
    cdef size_t rows
    if observed is not None:
        mask = np.ascontiguousarray(observed, dtype=np.uint32)
        rows = mask.shape[0]
        mask_p = <const uint32_t *> mask.data
    else:
        if n_rows is None:
            raise RuntimeError("sample_rows_many: neither n nor a mask tells "
                               "the number of rows")
        rows = n_rows
    if n_rows is not None and <size_t> n_rows != rows:
        raise RuntimeError("one mask per row")
    cdef const uint32_t ** cols = <const uint32_t **> malloc(
        sizeof(void *) * (n + 1))
    cdef uint32_t ** outs = <uint32_t **> malloc(sizeof(void *) * (n + 1))
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] w
    cdef SharedParams s
    words = []
    outw = []
    cdef int i
    for i in range(n):
        cols[i] = NULL
        if values is not None and values[i] is not None:
            s = first.shareds[i]
            w = value_words(s.c.kind, values[i])
            if <size_t> w.shape[0] != rows:
                free(cols)
                free(outs)
                raise RuntimeError("feature columns differ in length")
            words.append(w)
            cols[i] = <const uint32_t *> w.data
        w = np.zeros(max(rows, 1), np.uint32)
        outw.append(w)
        outs[i] = <uint32_t *> w.data
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] group = np.zeros(
        max(rows, 1), np.uint32)
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] member = np.zeros(
        max(rows, 1), np.uint32)
    cdef cnp.ndarray[cnp.float32_t, ndim=1] base = np.zeros(
        max(rows, 1), np.float32)
    cdef uint64_t db = <uint64_t> draw_base
    cdef bint no_values = values is None
    cdef dist_gibbs_t ** ptrs
    cdef int rc
    try:
        ptrs = _engine_ptrs(engines)
    except Exception:
        free(cols)
        free(outs)
        raise
    with nogil:
        rc = dist_gibbs_sample_rows_many(
            <dist_gibbs_t * const *> ptrs, m, rows,
            NULL if no_values else cols, mask_p, outs,
            <uint32_t *> group.data, <uint32_t *> member.data,
            <float *> base.data, seed_state, member_seed_state, db, flags)
    free(ptrs)
    free(cols)
    free(outs)
    check(rc)
    out_cols = []
    for i in range(n):
        s = first.shareds[i]
        w = outw[i][:rows]
        out_cols.append(w.view(np.float32) if s.c.kind == DIST_NICH else w)
    return out_cols, group[:rows], member[:rows], base[:rows]


def marginals_many_dev(engines, value_ptrs, size_t n_rows, masks,
                       size_t logp_ptr, size_t members_ptr=0,
                       size_t members_ld=0, bint prior_totals=True,
                       bint single=False):
    """The log marginals of feature subsets over M engines
    (dist_gibbs_marginals_many_dev; single: dist_gibbs_marginals_dev on the
    one engine): engines = GibbsEngine objects, value_ptrs device addresses of
    one column of n_rows words per feature (0 for a feature no mask names),
    masks a host list of uint32, the other pointers device addresses or 0.
    -> the engines' prior totals (numpy float32), or None"""
    cdef size_t m = len(engines)
    if m == 0 or engines[0] is None:
        raise RuntimeError("marginals_many: no engine" if m == 0
                           else "null engine")
    cdef GibbsEngine first = engines[0]
    cdef size_t nf = len(value_ptrs)
    if nf != len(first.shareds):
        raise RuntimeError("one value column per feature")
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] mk = np.ascontiguousarray(
        masks, dtype=np.uint32).reshape(-1)
    cdef size_t n_masks = mk.shape[0]
    cdef const uint32_t * mk_p = <const uint32_t *> mk.data
    cdef const uint32_t ** cols = <const uint32_t **> malloc(
        sizeof(void *) * (nf + 1))
    cdef size_t i
    cdef size_t addr
    for i in range(nf):
        addr = value_ptrs[i]
        cols[i] = <const uint32_t *> addr
    cdef cnp.ndarray[cnp.float32_t, ndim=1] totals = np.zeros(m, np.float32)
    cdef float * tp = <float *> totals.data if prior_totals else NULL
    cdef dist_gibbs_t ** ptrs
    cdef int rc
    try:
        ptrs = _engine_ptrs(engines)
    except Exception:
        free(cols)
        raise
    if single and m != 1:
        free(ptrs)
        free(cols)
        raise RuntimeError("marginals: one engine")
    with nogil:
        if single:
            rc = dist_gibbs_marginals_dev(ptrs[0], n_rows, cols, mk_p,
                                          n_masks, <float *> logp_ptr)
        else:
            rc = dist_gibbs_marginals_many_dev(
                <dist_gibbs_t * const *> ptrs, m, n_rows, cols, mk_p, n_masks,
                <float *> logp_ptr, <float *> members_ptr, members_ld, tp)
    free(ptrs)
    free(cols)
    check(rc)
    return totals.copy() if prior_totals and not single else None


def marginals_many(engines, values, masks, bint members=False,
                   bint single=False):
    """The log marginals of feature subsets over M engines, from host arrays
    (dist_gibbs_marginals_many; single: dist_gibbs_marginals on the one
    engine): values is one array per feature (None for a feature no mask
    names), masks a list of uint32.
    -> (logp [n, S], members_logp [M, n, S] or None, prior_totals [M] or
    None)"""
    cdef size_t m = len(engines)
    if m == 0 or engines[0] is None:
        raise RuntimeError("marginals_many: no engine" if m == 0
                           else "null engine")
    cdef GibbsEngine first = engines[0]
    cdef int n = len(first.shareds)
    if len(values) != n:
        raise RuntimeError("one value column per feature")
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] mk = np.ascontiguousarray(
        masks, dtype=np.uint32).reshape(-1)
    cdef size_t n_masks = mk.shape[0]
    cdef const uint32_t * mk_p = <const uint32_t *> mk.data
    cdef const uint32_t ** cols = <const uint32_t **> malloc(
        sizeof(void *) * (n + 1))
    cdef cnp.ndarray[cnp.uint32_t, ndim=1] w
    cdef SharedParams s
    words = []
    cdef int i
    cdef Py_ssize_t rows = -1
    try:
        for i in range(n):
            cols[i] = NULL
            if values[i] is None:
                continue
            s = first.shareds[i]
            w = value_words(s.c.kind, values[i])
            if rows >= 0 and w.shape[0] != rows:
                raise RuntimeError("feature columns differ in length")
            rows = w.shape[0]
            words.append(w)
            cols[i] = <const uint32_t *> w.data
        if rows < 0:
            raise RuntimeError("marginals_many: no column tells the number "
                               "of rows")
    except Exception:
        free(cols)
        raise
    cdef size_t n_rows = rows
    cdef size_t cells = max(n_masks, 1)
    cdef cnp.ndarray[cnp.float32_t, ndim=2] logp = np.zeros(
        (rows, cells), np.float32)
    cdef cnp.ndarray[cnp.float32_t, ndim=3] planes = np.zeros(
        (m if members else 1, rows if members else 1,
         cells if members else 1), np.float32)
    cdef cnp.ndarray[cnp.float32_t, ndim=1] totals = np.zeros(m, np.float32)
    cdef float * pp = <float *> planes.data if members else NULL
    cdef dist_gibbs_t ** ptrs
    cdef int rc
    try:
        ptrs = _engine_ptrs(engines)
    except Exception:
        free(cols)
        raise
    if single and m != 1:
        free(ptrs)
        free(cols)
        raise RuntimeError("marginals: one engine")
    with nogil:
        if single:
            rc = dist_gibbs_marginals(ptrs[0], n_rows, cols, mk_p, n_masks,
                                      <float *> logp.data)
        else:
            rc = dist_gibbs_marginals_many(
                <dist_gibbs_t * const *> ptrs, m, n_rows, cols, mk_p, n_masks,
                <float *> logp.data, pp, n_rows * cells,
                <float *> totals.data)
    free(ptrs)
    free(cols)
    check(rc)
    return (logp, planes if members else None,
            None if single else totals)


def relate_many(engines, size_t n_samples, uint32_t seed_state,
                uint32_t member_seed_state, draw_base=0, bint single=False):
    """Mutual information of every feature pair and the entropies under the
    predictive of M engines (dist_gibbs_relate_many; single: dist_gibbs_relate
    on the one engine) -> (mi [F, F] float64, stderr [F, F] float64,
    moments [F, F, 2] float64: the sums of d and of d^2)"""
    cdef size_t m = len(engines)
    if m == 0 or engines[0] is None:
        raise RuntimeError("relate_many: no engine" if m == 0
                           else "null engine")
    cdef GibbsEngine first = engines[0]
    cdef size_t nf = len(first.shareds)
    cdef cnp.ndarray[cnp.float64_t, ndim=2] mi = np.zeros((nf, nf),
                                                          np.float64)
    cdef cnp.ndarray[cnp.float64_t, ndim=2] se = np.zeros((nf, nf),
                                                          np.float64)
    cdef cnp.ndarray[cnp.float64_t, ndim=3] mo = np.zeros((nf, nf, 2),
                                                          np.float64)
    cdef uint64_t db = <uint64_t> draw_base
    cdef dist_gibbs_t ** ptrs = _engine_ptrs(engines)
    cdef int rc
    if single and m != 1:
        free(ptrs)
        raise RuntimeError("relate: one engine")
    with nogil:
        if single:
            rc = dist_gibbs_relate(ptrs[0], n_samples, seed_state,
                                   member_seed_state, db, <double *> mi.data,
                                   <double *> se.data, <double *> mo.data)
        else:
            rc = dist_gibbs_relate_many(
                <dist_gibbs_t * const *> ptrs, m, n_samples, seed_state,
                member_seed_state, db, <double *> mi.data, <double *> se.data,
                <double *> mo.data)
    free(ptrs)
    check(rc)
    return mi, se, mo
