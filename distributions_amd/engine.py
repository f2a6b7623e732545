"""The batched row engine: many Gibbs row updates per launch.

`Gibbs` is the reference's pattern -- one PitmanYor driver, one slave mixture
per feature column, one MixtureIdTracker (examples/mixture/main.py:59-123,
213-248) -- over a table of rows resident in HBM.  `ShardedGibbs` runs it with
one process per GPU: rows are block-partitioned, every rank keeps a replica of
the sufficient statistics, and each sub-sweep ends with one all-reduce of the
integer statistic deltas (RCCL over xGMI through torch.distributed).
"""
import numpy as np

from . import _core

KIND = {"dd": _core.KIND_DD, "bb": _core.KIND_BB, "gp": _core.KIND_GP,
        "nich": _core.KIND_NICH, "dpd": _core.KIND_DPD,
        "bnb": _core.KIND_BNB}


def dd_shared(alphas):
    """DirichletDiscrete::Shared (models/dd.hpp:57-86)"""
    return _core.SharedParams.make(_core.KIND_DD, alphas=list(alphas))


def bb_shared(alpha, beta):
    """BetaBernoulli::Shared (models/bb.hpp:54-76)"""
    return _core.SharedParams.make(_core.KIND_BB, p=(alpha, beta))


def gp_shared(alpha, inv_beta):
    """GammaPoisson::Shared (models/gp.hpp:52-81)"""
    return _core.SharedParams.make(_core.KIND_GP, p=(alpha, inv_beta))


def nich_shared(mu, kappa, sigmasq, nu):
    """NormalInverseChiSq::Shared (models/nich.hpp:52-95)"""
    return _core.SharedParams.make(_core.KIND_NICH,
                                   p=(mu, kappa, sigmasq, nu))


def bnb_shared(alpha, beta, r):
    """BetaNegativeBinomial::Shared (models/bnb.hpp:50-84)"""
    return _core.SharedParams.make(_core.KIND_BNB,
                                   p=(alpha, beta, float(int(r))))


def dpd_shared(alpha, betas, beta0=0.0):
    """DirichletProcessDiscrete::Shared with values remapped to 0..len(betas)-1
    (models/dpd.hpp:59-153)"""
    return _core.SharedParams.make(_core.KIND_DPD, p=(alpha, beta0),
                                   betas=np.asarray(betas, np.float32))


class Gibbs(object):
    """Clustering driver + feature slaves over resident rows.  The clustering
    model is PitmanYor(alpha, d), or LowEntropy(dataset_size) when
    `dataset_size` is given (alpha and d are then ignored)."""

    def __init__(self, alpha, d, shareds, dataset_size=None):
        self.alpha = float(alpha)
        self.d = float(d)
        self.dataset_size = dataset_size
        self.shareds = list(shareds)
        self.core = _core.GibbsEngine(self.alpha, self.d, self.shareds,
                                      dataset_size)

    # -- data ---------------------------------------------------------------
    def load_rows(self, values, assign_packed, nonempty_groups,
                  empty_groups=1, row_offset=0):
        self.core.load_rows(values, assign_packed, nonempty_groups,
                            empty_groups, row_offset)

    def load_rows_torch(self, values, assign_packed, nonempty_groups,
                        empty_groups=1, row_offset=0):
        """values: int32/float32 CUDA tensors (one per feature);
        assign_packed: int32 CUDA tensor, rewritten in place to global ids."""
        ptrs = [int(v.data_ptr()) for v in values]
        self.core.load_rows_dev(ptrs, int(assign_packed.data_ptr()),
                                int(assign_packed.numel()), nonempty_groups,
                                empty_groups, row_offset,
                                keep=(list(values), assign_packed))

    def load_rows_unassigned(self, values, empty_groups=1, row_offset=0):
        """Rows without a group yet (a fresh mixture, examples/mixture/
        main.py:222-224); `init_sequential` assigns them."""
        self.core.load_rows_unassigned(values, empty_groups, row_offset)

    def init_sequential(self, row_begin, row_end, rng_state, prior_only=False):
        """The initialisation loop of examples/mixture/main.py on the
        device: rows [row_begin, row_end) are added one at a time -- score
        every group (all features, main.py:265-270; `prior_only`: the
        clustering model alone, main.py:227-232), sample, add.  Rows are
        assigned in order, starting at the first unassigned one.  Returns the
        new rng state."""
        return self.core.init_sequential(row_begin, row_end, rng_state,
                                         prior_only)

    # -- sweeps -------------------------------------------------------------
    def sweep(self, row_begin, row_end, batch_rows, seed, draw_base=0):
        """One pass over rows [row_begin,row_end) in frozen batches.

        Where the group set is normalised on the device (one feature with
        integer statistics: the default) the pass is QUEUED when this returns;
        the next sweep goes on without the host, and any other call on the
        engine (counts(), assignments(), ...) first waits for the device and
        pulls the host's copy of the group set.  `_core.synchronize()` waits
        explicitly."""
        self.core.sweep(row_begin, row_end, batch_rows, _core.rng_seed(seed),
                        draw_base)

    def sweep_sequential(self, row_begin, row_end, rng_state):
        """The reference's sequential chain; returns the new rng state."""
        return self.core.sweep_sequential(row_begin, row_end, rng_state)

    # -- state --------------------------------------------------------------
    def __len__(self):
        return self.core.group_count()

    def counts(self):
        return self.core.counts()

    def assignments(self):
        return self.core.assignments()

    def get_group(self, feature, groupid):
        return self.core.get_group(feature, groupid)

    def validate(self, raise_on_failure=True):
        """Mixture::validate for the whole engine (mixture.hpp:152-163,
        440-444): statistics against a recount from the rows, on the device
        (dist_gibbs_validate).  Returns the report; raises RuntimeError on
        the first inconsistency."""
        return self.core.validate(raise_on_failure)

    def row_scores(self, row):
        return self.core.row_scores(row)

    # -- held-out rows ------------------------------------------------------
    _PREDICT_MODES = {"sample": 0, "map": 1, None: None}

    def predict(self, values, mode="sample", seed=0, draw_base=0):
        """Rows that are NOT in the table, against the current state.
        values: one host array per feature.  -> (logp, groups, prior_total):
        logp[q] = log_sum_exp over all groups, empty ones included, of the
        clustering model's score_value plus every feature's (mixture.hpp:
        416-425, random.cc:78-92) -- under PitmanYor the log posterior
        predictive density of row q; under LowEntropy, whose scores are not
        normalised, subtract prior_total (log_sum_exp of the clustering
        model's scores alone).  groups[q] is the row's group as a global id:
        mode "sample" draws it with engine step draw_base + q + 1 of `seed`
        (the batch's convention), "map" takes the first group of maximal
        score, None leaves it out (groups is None).  Nothing in the engine
        changes."""
        return self.core.predict(list(values), self._PREDICT_MODES[mode],
                                 _core.rng_seed(seed), draw_base)

    def predict_torch(self, values, mode="sample", seed=0, draw_base=0):
        """predict for device tensors (one 4-byte-per-row CUDA tensor per
        feature): the results are tensors on the same device and nothing is
        staged through the host.  -> (logp, groups, prior_total)"""
        import torch
        values = [v.contiguous() for v in values]
        n = int(values[0].numel())
        m = self._PREDICT_MODES[mode]
        dev = values[0].device
        logp = torch.empty(n, dtype=torch.float32, device=dev)
        groups = (torch.empty(n, dtype=torch.int32, device=dev)
                  if m is not None else None)
        # (the library works on its own stream: what filled the tensors on
        # torch's must be done)
        torch.cuda.current_stream(dev).synchronize()
        total = self.core.predict_dev(
            [int(v.data_ptr()) for v in values], n, int(logp.data_ptr()),
            int(groups.data_ptr()) if groups is not None else 0,
            0 if m is None else m, _core.rng_seed(seed), draw_base)
        return logp, groups, total

    def responsibilities(self, values):
        """The group posterior of rows that are NOT in the table -> float32
        [n, K], K = len(self): row q's `predict` scores through
        scores_to_likelihoods (random.cc:94-103), each likelihood times
        1.0f / total, the weights `predict(mode="sample")` draws row q's
        group with, slot by slot (empty groups included; a slot's global id
        is not part of it).  Nothing in the engine changes."""
        return _core.responsibilities(self.core, list(values)).T

    def responsibilities_torch(self, values):
        """responsibilities for device tensors -> a [n, K] tensor on the same
        device (a transposed view of the k-major planes the kernel writes)"""
        import torch
        values = _device_columns(values)
        n = int(values[0].numel())
        dev = values[0].device
        resp = torch.empty((len(self), n), dtype=torch.float32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        _core.responsibilities_dev(self.core,
                                   [int(v.data_ptr()) for v in values], n,
                                   int(resp.data_ptr()), n)
        return resp.t()

    def coassign(self, values, other=None):
        """coassign_many on this engine alone (dist_gibbs_coassign):
        out[a, b] = sum_k r_a[k] r_b[k] with r = `responsibilities`."""
        return _core.coassign_many([self.core], list(values),
                                   None if other is None else list(other),
                                   True)

    def coassign_torch(self, values, other=None):
        """coassign for device tensors -> a [n, n_other] tensor"""
        return _coassign_torch([self], values, other, True)

    def partition_agreement(self, extra=None, nlogn=True):
        """partition_agreement_many on this engine alone
        (dist_gibbs_partition_agreement): the resident assignments against
        the label columns of `extra`."""
        return _partition_agreement([self], extra, nlogn, True)

    def coassign_resident(self, rows, other=None):
        """coassign_resident_many on this engine alone
        (dist_gibbs_coassign_resident): 1.0 where the two resident rows share
        a group, else 0.0."""
        return _core.coassign_resident_many([self.core], rows, other, True)

    def coassign_resident_torch(self, rows, other=None):
        """coassign_resident for device index tensors -> a tensor"""
        return _coassign_resident_torch([self], rows, other, True)

    def coassign_topk(self, values, other=None, k=10, exclude_self=None):
        """coassign_topk_many on this engine alone
        (dist_gibbs_coassign_topk) -> (index int32 [n, k], prob [n, k])"""
        return _coassign_topk([self], values, other, k, exclude_self, True)

    def coassign_topk_torch(self, values, other=None, k=10,
                            exclude_self=None):
        """coassign_topk for device tensors -> two [n, k] tensors"""
        return _coassign_topk_torch([self], values, other, k, exclude_self,
                                    True)

    def search_resident(self, values, k=10, row_begin=0, row_end=None):
        """search_resident_many on this engine alone
        (dist_gibbs_search_resident) -> (index int32 [n, k], prob [n, k])"""
        return _search_resident([self], values, k, row_begin, row_end, True)

    def search_resident_torch(self, values, k=10, row_begin=0, row_end=None):
        """search_resident for device tensors -> two [n, k] tensors"""
        return _search_resident_torch([self], values, k, row_begin, row_end,
                                      True)

    def coassign_resident_topk(self, rows, k=10, exclude_self=True,
                               row_begin=0, row_end=None):
        """coassign_resident_topk_many on this engine alone
        (dist_gibbs_coassign_resident_topk): the k lowest-indexed rows of
        rows[a]'s own group, then of the others"""
        return _coassign_resident_topk([self], rows, k, exclude_self,
                                       row_begin, row_end, True)

    def coassign_resident_topk_torch(self, rows, k=10, exclude_self=True,
                                     row_begin=0, row_end=None):
        """coassign_resident_topk for a device index tensor"""
        return _coassign_resident_topk_torch([self], rows, k, exclude_self,
                                             row_begin, row_end, True)

    def predict_feature(self, values, target, candidates=None, observed=None,
                        mode="map", seed=0, draw_base=0, staged=True):
        """Given some cells of rows that are NOT in the table, the cell that
        is missing: feature `target`'s predictive given the others.
        values: one host array per feature (the target's may be None; words
        in unobserved cells are never read).  candidates: values of the
        target to score; None takes the whole domain of a DirichletDiscrete
        (0 .. dim-1), BetaBernoulli (0, 1) or DirichletProcessDiscrete
        (0 .. dim-1, then OTHER) target, the other kinds need a list.
        observed: one uint32 mask per row, bit f set when feature f of the
        row is observed (bit `target` is ignored); None: every other feature
        is observed.  -> (joint [n, C] float32, base [n] float32, choice [n]
        uint32 or None):
        joint[q, c] = log_sum_exp over all groups of the clustering model's
        score_value, the observed features' and the target's at
        candidates[c] (mixture.hpp:416-425, random.cc:78-92) -- the logp
        `predict` returns for the row completed with that candidate, when
        everything else is observed; base[q] the same with the target left
        out, the log marginal of the observed cells.  joint - base[:, None]
        is the log conditional of the target, under LowEntropy too.
        choice[q] indexes the candidates: mode "sample" draws it from joint[q]
        with engine step draw_base + q + 1 of `seed`, "map" takes the first
        maximum, None leaves it out.  staged=False scores every (row,
        candidate) pair from scratch (the same bits, slower where other
        features are observed).  Nothing in the engine changes."""
        return self.core.predict_feature(
            list(values), target, candidates, observed,
            self._PREDICT_MODES[mode], _core.rng_seed(seed), draw_base,
            0 if staged else _core.PREDICT_FEATURE_RECOMPUTE)

    def predict_feature_torch(self, values, target, candidates=None,
                              observed=None, mode="map", seed=0, draw_base=0,
                              staged=True):
        """predict_feature for device tensors (one 4-byte-per-row CUDA tensor
        per feature, the target's may be None; observed a CUDA int32 tensor
        or None; candidates stay a host list): the results are tensors on the
        same device and nothing is staged through the host.
        -> (joint, base, choice)"""
        import torch
        values = [None if v is None else v.contiguous() for v in values]
        given = [v for v in values if v is not None]
        if observed is not None:
            observed = observed.contiguous()
        ref = given[0] if given else observed
        n = int(ref.numel())
        dev = ref.device
        m = self._PREDICT_MODES[mode]
        C = len(self.core.feature_candidates(target, candidates))
        joint = torch.empty((n, C), dtype=torch.float32, device=dev)
        base = torch.empty(n, dtype=torch.float32, device=dev)
        choice = (torch.empty(n, dtype=torch.int32, device=dev)
                  if m is not None else None)
        # (the library works on its own stream: what filled the tensors on
        # torch's must be done)
        torch.cuda.current_stream(dev).synchronize()
        self.core.predict_feature_dev(
            [0 if v is None else int(v.data_ptr()) for v in values], n,
            0 if observed is None else int(observed.data_ptr()), target,
            candidates, int(joint.data_ptr()), int(base.data_ptr()),
            int(choice.data_ptr()) if choice is not None else 0,
            0 if m is None else m, _core.rng_seed(seed), draw_base,
            0 if staged else _core.PREDICT_FEATURE_RECOMPUTE)
        return joint, base, choice

    def marginals(self, values, masks):
        """marginals_many on this engine alone (dist_gibbs_marginals)
        -> logp float32 [n, S]: no fold and no - log M.  logp[q, s] is
        `predict_feature(values, target=t, observed=[masks[s]] * n,
        mode=None)`'s base for any t outside masks[s], for the mask of all
        features `predict`'s logp, for mask 0 its prior_total -- bit for bit
        under PitmanYor; under LowEntropy each minus prior_total (one float
        subtraction), which makes it a proper log density."""
        return _core.marginals_many([self.core], list(values), masks, False,
                                    True)[0]

    def marginals_torch(self, values, masks):
        """marginals for device tensors -> a [n, S] tensor"""
        return _marginals_torch([self], values, masks, False, True)[0]

    def relate(self, n_samples, seed=0, member_seed=None, draw_base=0,
               moments=False):
        """relate_many on this engine alone (dist_gibbs_relate): the rows are
        `sample_rows_many([self], n_samples, ...)`'s, which are
        `sample_rows`', scored by `marginals` (no fold).
        -> (mi [F, F] float64, stderr [F, F] float64)"""
        if member_seed is None:
            member_seed = seed + 1
        out = _core.relate_many([self.core], n_samples, _core.rng_seed(seed),
                                _core.rng_seed(member_seed), draw_base, True)
        return out if moments else out[:2]

    def sample_rows(self, n=None, values=None, observed=None, seed=0,
                    draw_base=0):
        """Rows that are NOT in the table, drawn from the mixture: synthetic
        rows, or the joint completion of rows with holes.
        observed: one uint32 mask per row, bit f set when feature f of the
        row is observed (required when `values` is given); None: nothing is
        observed and `n` rows are drawn.  values: one host array per feature
        (None for a feature no row observes; words in unobserved cells are
        never read).  -> (columns, groups): per row q a group (a global id)
        drawn from the clustering model's score_value folded with the
        observed features' (mixture.hpp:416-425) with engine step
        draw_base + q + 1 of `seed` -- predict(mode="sample")'s group when
        everything is observed -- and then EVERY unobserved cell drawn from
        that one group's posterior predictive (Group::sample_value), so the
        cells of a row fit together; observed cells come back as given.
        columns[f] is float32 for NormalInverseChiSq, uint32 otherwise
        (0xFFFFFFFF: a DirichletProcessDiscrete value outside the table).
        Cell (q, f) depends on (seed, draw_base + q, f) alone: calls over
        disjoint draw_base ranges are independent.  Nothing in the engine
        changes."""
        return self.core.sample_rows(n, None if values is None
                                     else list(values), observed,
                                     _core.rng_seed(seed), draw_base)

    def sample_rows_torch(self, n=None, values=None, observed=None, seed=0,
                          draw_base=0, out=None):
        """sample_rows for device tensors (values: one 4-byte-per-row CUDA
        tensor per feature or None; observed a CUDA int32 tensor or None):
        the results are tensors on the same device (the current one when
        nothing is given) and nothing is staged through the host.  out: the
        tensors to fill, one per feature; out[f] may be values[f] itself,
        which completes the rows in place (only unobserved cells are
        written).  -> (columns, groups)"""
        import torch
        if values is not None and observed is None:
            raise RuntimeError("sample_rows: values need an observed mask")
        if observed is not None:
            observed = observed.contiguous()
            n = int(observed.numel())
            dev = observed.device
        else:
            values = None
            dev = torch.device("cuda", torch.cuda.current_device())
        if values is not None:
            values = [None if v is None else v.contiguous() for v in values]
        if out is None:
            out = [torch.empty(n, dtype=torch.float32
                               if s.kind == _core.KIND_NICH else torch.int32,
                               device=dev) for s in self.shareds]
        groups = torch.empty(n, dtype=torch.int32, device=dev)
        # (the library works on its own stream: what filled the tensors on
        # torch's must be done)
        torch.cuda.current_stream(dev).synchronize()
        self.core.sample_rows_dev(
            None if values is None
            else [0 if v is None else int(v.data_ptr()) for v in values], n,
            0 if observed is None else int(observed.data_ptr()),
            [int(o.data_ptr()) for o in out], int(groups.data_ptr()),
            _core.rng_seed(seed), draw_base)
        return out, groups

    # -- hyper-parameters ---------------------------------------------------
    # The step the reference alternates with assignment sweeps
    # (mixture.hpp:427-438, then sample_from_scores and init()), on the
    # statistics the engine holds.  Scoring closes an open run but changes
    # nothing; set_* and sample_* install new values and rebuild what is
    # derived from them.  self.shareds, self.alpha and self.d follow.
    def score_data(self):
        """-> (score_data per feature, score_counts of the clustering model)"""
        return self.core.score_data()

    def score_data_grid(self, feature, shareds):
        """score_data of `feature` under each candidate Shared"""
        return self.core.score_data_grid(feature, list(shareds))

    def score_counts_grid(self, alphas, ds):
        """PitmanYor score_counts under each (alphas[c], ds[c])"""
        return self.core.score_counts_grid(alphas, ds)

    def set_shared(self, feature, shared):
        self.core.set_shared(feature, shared)
        self.shareds[feature] = shared

    def set_clustering(self, alpha, d):
        self.core.set_clustering(alpha, d)
        self.alpha, self.d = self.core.clustering()

    def sample_hypers(self, feature, shareds, rng_state):
        """Score the grid, draw one candidate with one engine step, install
        it -- all on the device.  -> (index, new rng state)"""
        shareds = list(shareds)
        index, rng_state = self.core.sample_hypers(feature, shareds, rng_state)
        self.shareds[feature] = shareds[index]
        return index, rng_state

    def sample_hypers_pass(self, feature, grids, rng_state, coords=None):
        """A whole coordinate pass of a DirichletDiscrete feature in one
        call: for step i, alphas[coords[i]] is given each value of grids[i]
        (float32 [n_coords, G], or one row [G] for every step), one is drawn
        with one engine step and takes its place before the next step.
        coords: any order, repeats allowed; default 0 .. dim-1.  Bit for bit
        the loop of sample_hypers calls over coordinate grids, in two launches
        and one install where the device can reproduce it (hyper_stats tells).
        -> (indices uint32 [n_coords], new rng state)"""
        indices, rng_state = self.core.sample_hypers_pass(feature, grids,
                                                          rng_state, coords)
        self.shareds[feature] = self.core.shared(feature)
        return indices, rng_state

    def sample_clustering(self, alphas, ds, rng_state):
        """-> (index, new rng state); (alphas[index], ds[index]) installed"""
        index, rng_state = self.core.sample_clustering(alphas, ds, rng_state)
        self.alpha, self.d = self.core.clustering()
        return index, rng_state

    def hyper_stats(self):
        """(accumulator chains, candidates scored, launches, calls)"""
        return self.core.hyper_stats()

    def kernel_stats(self, reset=False):
        return self.core.kernel_stats(reset)

    def set_option(self, name, value):
        self.core.set_option(name, value)

    def path_counts(self):
        return self.core.path_counts()


def sweep_sequential_many(engines, row_begin, row_end, rng_states):
    """M independent exact chains in ONE launch (BASELINE configs[3]:
    "independent chains"): engine i -- a `Gibbs` with its own rows -- runs the
    reference's sequential chain (examples/mixture/main.py:236-244) over its
    rows [row_begin, row_end) with rng_states[i]; one workgroup per chain,
    group creation and removal on the device.  The engines share one feature
    list.  -> the new rng states (numpy uint32)."""
    return _core.sweep_sequential_many([g.core for g in engines], row_begin,
                                       row_end, rng_states)


def sample_hypers_pass_many(engines, feature, grids, rng_states, coords=None):
    """Gibbs.sample_hypers_pass on M engines -- `Gibbs` objects whose feature
    `feature` is DirichletDiscrete of one dim -- in the same two launches,
    engine i with rng_states[i]; the grid's accumulator chains are shared.
    -> (indices uint32 [M, n_coords], the new rng states uint32 [M])"""
    indices, states = _core.sample_hypers_pass_many(
        [g.core for g in engines], feature, grids, rng_states, coords)
    for g in engines:
        g.shareds[feature] = g.core.shared(feature)
    return indices, states


PREDICT_MANY_DRAW_ALL = _core.PREDICT_MANY_DRAW_ALL


def _cores(engines):
    return [None if g is None else g.core for g in engines]


def predict_many(engines, values, mode="sample", seed=0, member_seed=None,
                 draw_base=0, members=False, flags=0):
    """Rows that are NOT in the table, against M engines at once: the
    predictive averaged over the members of an ensemble (the chains of
    sweep_sequential_many, each one posterior sample), in launches that cover
    every member.  values: one host array per feature.
    -> (logp, members, groups, members_logp, prior_totals):
    logp[q] = log (1/M) sum_e p(x_q | engine e), the in-order log_sum_exp
    (random.cc:78-92) over the engines of `Gibbs.predict`'s logp -- under
    LowEntropy each normalised by its own prior_total first -- minus
    fast_log(M); members[q] is the engine drawn from those M values with
    engine step draw_base + q + 1 of `member_seed` (None: seed + 1), or for
    mode "map" the first engine of maximal value; groups[q] is the group
    engines[members[q]].predict(values, mode, seed, draw_base) gives row q,
    as that engine's global id; mode None leaves both out.  members_logp
    (members=True) is the [M, n] array the fold ran over, prior_totals the
    engines' prior totals.  The engines share one feature list and one
    clustering model; nothing in them changes."""
    if member_seed is None:
        member_seed = seed + 1
    return _core.predict_many(_cores(engines), list(values),
                              Gibbs._PREDICT_MODES[mode],
                              _core.rng_seed(seed),
                              _core.rng_seed(member_seed), draw_base, members,
                              flags)


def predict_many_torch(engines, values, mode="sample", seed=0,
                       member_seed=None, draw_base=0, members=False, flags=0):
    """predict_many for device tensors (one 4-byte-per-row CUDA tensor per
    feature): the results but prior_totals (numpy) are tensors on the same
    device and nothing is staged through the host."""
    import torch
    if member_seed is None:
        member_seed = seed + 1
    values = [v.contiguous() for v in values]
    n = int(values[0].numel())
    m = Gibbs._PREDICT_MODES[mode]
    dev = values[0].device
    logp = torch.empty(n, dtype=torch.float32, device=dev)
    chosen = groups = planes = None
    if m is not None:
        chosen = torch.empty(n, dtype=torch.int32, device=dev)
        groups = torch.empty(n, dtype=torch.int32, device=dev)
    if members:
        planes = torch.empty((len(engines), n), dtype=torch.float32,
                             device=dev)
    # (the library works on its own stream: what filled the tensors on
    # torch's must be done)
    torch.cuda.current_stream(dev).synchronize()
    totals = _core.predict_many_dev(
        _cores(engines), [int(v.data_ptr()) for v in values], n,
        int(logp.data_ptr()),
        int(chosen.data_ptr()) if chosen is not None else 0,
        int(groups.data_ptr()) if groups is not None else 0,
        0 if m is None else m, _core.rng_seed(seed),
        _core.rng_seed(member_seed), draw_base,
        int(planes.data_ptr()) if planes is not None else 0, n, True, flags)
    return logp, chosen, groups, planes, totals


def coassign_many(engines, values, other=None):
    """Which rows belong together: for rows that are NOT in the table, the
    probability that `predict(mode="sample")` puts row a of `values` and row
    b of `other` (None: of `values` itself) into the same slot when the
    engine is drawn uniformly from `engines` and the two draws are
    independent.  -> float32 [n, n_other]:
    out[a, b] = (1/M) sum_e sum_k r_e,a[k] r_e,b[k], r_e = engine e's
    `responsibilities`, as ONE float fmaf chain per cell (engines in order,
    slots in order) divided by float(M); with other=None symmetric bit for
    bit.  It is NOT the joint law in which a joining a group changes b's
    predictive, and empty slots count as distinct groups: with several empty
    groups the new-group mass divides among them.  Cells of a row whose logp
    is not finite are unspecified.  The engines share one feature list and
    one clustering model; nothing in them changes."""
    return _core.coassign_many(_cores(engines), list(values),
                               None if other is None else list(other))


def _device_columns(values, dev=None):
    """device tensors as the library reads them: contiguous, 4 bytes per
    row, one length, all on one CUDA device (`dev` if given)"""
    values = [v.contiguous() for v in values]
    if not values:
        raise RuntimeError("one value column per feature")
    dev = values[0].device if dev is None else dev
    for v in values:
        if not v.is_cuda or v.device != dev:
            raise RuntimeError("value columns on one CUDA device")
        if v.element_size() != 4:
            raise RuntimeError("value columns of 4 bytes per row")
        if v.numel() != values[0].numel():
            raise RuntimeError("feature columns differ in length")
    return values


def _coassign_torch(engines, values, other, single):
    import torch
    values = _device_columns(values)
    n_q = int(values[0].numel())
    dev = values[0].device
    t_ptrs, n_t = None, n_q
    if other is not None:
        other = _device_columns(other, dev)
        n_t = int(other[0].numel())
        t_ptrs = [int(v.data_ptr()) for v in other]
    out = torch.empty((n_q, n_t), dtype=torch.float32, device=dev)
    # (the library works on its own stream: what filled the tensors on
    # torch's must be done)
    torch.cuda.current_stream(dev).synchronize()
    _core.coassign_many_dev(_cores(engines),
                            [int(v.data_ptr()) for v in values], n_q, t_ptrs,
                            n_t, int(out.data_ptr()), n_t, single)
    return out


def coassign_many_torch(engines, values, other=None):
    """coassign_many for device tensors (one 4-byte-per-row CUDA tensor per
    feature) -> a [n, n_other] tensor on the same device; nothing is staged
    through the host."""
    return _coassign_torch(engines, values, other, False)


# -- resident rows: what M chains say about the rows they hold ---------------
class PartitionAgreement(object):
    """What the device computes about P partitions of the same n rows, the
    first m of them engines' resident assignments: sq[a, b] = the sum of the
    squared cells of the contingency table of a and b (uint64 [P, P]) and
    nlogn[a, b] = the sum of n log n over its cells (float64 [P, P], or
    None).  The measures below are host arithmetic on the two."""

    def __init__(self, sq, nlogn, n, m):
        self.sq = sq
        self.nlogn = nlogn
        self.n = int(n)
        self.m = int(m)

    def __getitem__(self, key):
        return getattr(self, key)


def _is_tensor(c):
    return hasattr(c, "data_ptr")


def _label_bounds(columns, n_labels):
    """n_labels per column; None: max + 1"""
    if n_labels is not None:
        if np.ndim(n_labels) == 0:
            n_labels = [n_labels] * len(columns)
        return [int(k) for k in n_labels]
    return [(int(c.max()) + 1 if len(c) else 0) for c in columns]


def _partition_agreement(engines, extra, nlogn, single, n_labels=None):
    extra = [] if extra is None else list(extra)
    if not engines and not extra:
        raise RuntimeError("partition_agreement: no partition")
    if any(g is None for g in engines):
        raise RuntimeError("null engine")
    dev = bool(extra) and all(_is_tensor(c) for c in extra)
    if extra and not dev and any(_is_tensor(c) for c in extra):
        raise RuntimeError("partition_agreement: label columns either all "
                           "host arrays or all CUDA tensors")
    if dev:
        import torch
        cols = []
        for c in extra:
            if not c.is_cuda or c.device != extra[0].device:
                raise RuntimeError("label columns on one CUDA device")
            if c.is_floating_point() or c.is_complex() or (
                    c.dtype == torch.bool):
                raise RuntimeError("label columns of integers")
            if c.numel() and c.element_size() != 4 and (
                    int(c.min()) < 0 or int(c.max()) > 0xFFFFFFFF):
                raise RuntimeError("partition_agreement: label outside 32 "
                                   "bits")
            if c.element_size() != 4:
                c = c.to(torch.int32)
            cols.append(c.contiguous().reshape(-1))
        bounds = _label_bounds(cols, n_labels)
        lengths = [int(c.numel()) for c in cols]
        # (the library works on its own stream: what filled the tensors on
        # torch's must be done)
        torch.cuda.current_stream(cols[0].device).synchronize()
        handles = [int(c.data_ptr()) for c in cols]
    else:
        cols = [np.asarray(c).reshape(-1) for c in extra]
        for c in cols:
            if c.size and (c.min() < 0 or c.max() > 0xFFFFFFFF):
                raise RuntimeError("partition_agreement: label outside 32 "
                                   "bits")
        bounds = _label_bounds(cols, n_labels)
        lengths = [int(c.size) for c in cols]
        handles = cols
    n = engines[0].core.row_count() if engines else lengths[0]
    for a, length in enumerate(lengths):
        if length != n:
            raise RuntimeError(
                "partition_agreement: extra column %d has %d rows, not %d"
                % (a, length, n))
    if len(bounds) != len(cols):
        raise RuntimeError("partition_agreement: one n_labels per column")
    sq, nl = _core.partition_agreement_many(
        [g.core for g in engines], n, handles, bounds, nlogn, dev, single)
    return PartitionAgreement(sq, nl, n, len(engines))


def partition_agreement_many(engines, extra=None, nlogn=True):
    """Have the chains mixed, and which clustering do I report: the agreement
    of the RESIDENT partitions of M engines -- `Gibbs` objects that hold the
    same rows in the same order, which the caller vouches for -- and of the
    label columns of `extra` (a ground truth, an earlier `assignments()`;
    host arrays or CUDA tensors, bins up to max + 1).  -> a
    `PartitionAgreement` over the P = M + len(extra) partitions, engines
    first: sq exact, nlogn (None with nlogn=False) equal in every bit between
    equal calls.  `rand_index`, `adjusted_rand_index`, `binder_distance`,
    `variation_of_information` and `consensus` read it.  The engines are read
    as `assignments()` reads them and nothing in them changes; a partition
    may have at most 18 432 groups."""
    return _partition_agreement(list(engines), extra, nlogn, False)


def partition_agreement_labels(labels, n_labels=None, nlogn=True):
    """partition_agreement_many for plain label columns and no engine
    (dist_partition_agreement[_dev]): numpy arrays or CUDA tensors of one
    length; n_labels: an exclusive bound per column (default max + 1)."""
    return _partition_agreement([], labels, nlogn, False, n_labels)


def _pair_counts(res):
    """(T_ab, T_a as a column, C) in float64 from exact integers: the row
    pairs joined by both partitions, by one, and all"""
    sq = np.asarray(res.sq, np.uint64)
    n = int(res.n)
    t = ((sq - np.uint64(n)) // np.uint64(2)).astype(np.float64)
    return t, np.diag(t).copy(), n * (n - 1) / 2.0


def rand_index(res):
    """-> float64 [P, P]: (C - T_a - T_b + 2 T_ab) / C; 1.0 for n < 2"""
    t, ta, c = _pair_counts(res)
    if c == 0:
        return np.ones_like(t)
    return (c - ta[:, None] - ta[None, :] + 2.0 * t) / c


def adjusted_rand_index(res):
    """-> float64 [P, P]: (T_ab - E) / ((T_a + T_b) / 2 - E) with
    E = T_a T_b / C (Hubert and Arabie 1985); 1.0 where the denominator is 0
    or n < 2"""
    t, ta, c = _pair_counts(res)
    if c == 0:
        return np.ones_like(t)
    e = ta[:, None] * ta[None, :] / c
    den = (ta[:, None] + ta[None, :]) / 2.0 - e
    out = np.ones_like(t)
    np.divide(t - e, den, out=out, where=den != 0)
    return out


def binder_distance(res):
    """-> int64 [P, P]: sq_aa + sq_bb - 2 sq_ab, the ordered row pairs that
    one partition joins and the other separates"""
    sq = np.asarray(res.sq, np.uint64).astype(np.int64)
    d = np.diag(sq)
    return d[:, None] + d[None, :] - 2 * sq


def variation_of_information(res):
    """-> float64 [P, P]: (nlogn_aa + nlogn_bb - 2 nlogn_ab) / n, in nats"""
    if res.nlogn is None:
        raise RuntimeError("variation_of_information: the result was "
                           "computed with nlogn=False")
    nl = np.asarray(res.nlogn, np.float64)
    d = np.diag(nl)
    return (d[:, None] + d[None, :] - 2.0 * nl) / float(res.n)


def consensus(res, among=None):
    """The least-squares clustering (Dahl 2006) -> (index, total_distance):
    the member a of `among` (default: the m engines) with the smallest
    sum over b in `among` of binder_distance[a, b] -- the sample nearest to
    the posterior similarity matrix of those samples, which is never formed
    --, the first minimum on ties; total_distance[i] is the sum of
    among[i]."""
    among = (np.arange(res.m) if among is None
             else np.asarray(among, np.int64).reshape(-1))
    if among.size == 0:
        raise RuntimeError("consensus: no partition to choose among")
    d = binder_distance(res)[np.ix_(among, among)]
    total = d.sum(axis=1)
    return int(among[int(np.argmin(total))]), total


def coassign_resident_many(engines, rows, other=None):
    """The posterior similarity of chosen RESIDENT rows -> float32
    [len(rows), len(other)]: the fraction of `engines` in which rows[i] and
    other[j] (None: rows) carry the same group id; with other=None symmetric
    in every bit with a diagonal of 1.  The engines hold the same rows in the
    same order; nothing in them changes."""
    return _core.coassign_resident_many(_cores(engines), rows, other)


def _device_rows(t, dev=None):
    import torch
    if not t.is_cuda or (dev is not None and t.device != dev):
        raise RuntimeError("row indices on one CUDA device")
    if t.is_floating_point() or t.dtype == torch.bool:
        raise RuntimeError("row indices of integers")
    t = t.reshape(-1)
    # (4-byte words are read as unsigned: a negative int32 is out of range
    # for the library as well)
    if t.element_size() != 4:
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= 2 ** 31):
            raise RuntimeError("coassign_resident_many: row index outside "
                               "the engines' rows")
        t = t.to(torch.int32)
    return t.contiguous()


def _coassign_resident_torch(engines, rows, other, single):
    import torch
    ra = _device_rows(rows)
    dev = ra.device
    rb = None if other is None else _device_rows(other, dev)
    na = int(ra.numel())
    nb = na if rb is None else int(rb.numel())
    out = torch.empty((na, nb), dtype=torch.float32, device=dev)
    # (the library works on its own stream: what filled the tensors on
    # torch's must be done)
    torch.cuda.current_stream(dev).synchronize()
    _core.coassign_resident_many_dev(
        _cores(engines), int(ra.data_ptr()), na,
        0 if rb is None else int(rb.data_ptr()), nb, int(out.data_ptr()), nb,
        single)
    return out


def coassign_resident_many_torch(engines, rows, other=None):
    """coassign_resident_many for device index tensors -> a [n, n_other]
    tensor on the same device; nothing is staged through the host."""
    return _coassign_resident_torch(engines, rows, other, False)


def _coassign_topk_flags(other, exclude_self):
    if exclude_self is None:
        exclude_self = other is None
    return _core.COASSIGN_EXCLUDE_SELF if exclude_self else 0


def _coassign_topk(engines, values, other, k, exclude_self, single):
    index, prob = _core.coassign_topk_many(
        _cores(engines), list(values),
        None if other is None else list(other), k,
        _coassign_topk_flags(other, exclude_self), single)
    return index.view(np.int32), prob


def coassign_topk_many(engines, values, other=None, k=10, exclude_self=None):
    """Search and de-duplication over rows that are NOT in the table: for
    every row a of `values`, the k rows b of `other` (None: of `values`
    itself) it most likely shares a slot with -- the k largest cells of
    `coassign_many`'s row a, bit for bit, without the [n, n_other] matrix.
    -> (index int32 [n, k], prob float32 [n, k]): targets by cell descending,
    among bit-equal cells by index ascending; where fewer than k targets are
    eligible the rest is index -1 and probability +0.  exclude_self leaves
    b == a out; None means `other is None`, and True with `other` given fails.
    k is at most 128.  A row of `values` whose logp is not finite has an
    unspecified result row; such a row among the targets leaves the whole
    result unspecified."""
    return _coassign_topk(engines, values, other, k, exclude_self, False)


def _coassign_topk_torch(engines, values, other, k, exclude_self, single):
    import torch
    values = _device_columns(values)
    n_q = int(values[0].numel())
    dev = values[0].device
    t_ptrs, n_t = None, n_q
    if other is not None:
        other = _device_columns(other, dev)
        n_t = int(other[0].numel())
        t_ptrs = [int(v.data_ptr()) for v in other]
    k = int(k)
    index = torch.empty((n_q, k), dtype=torch.int32, device=dev)
    prob = torch.empty((n_q, k), dtype=torch.float32, device=dev)
    # (the library works on its own stream: what filled the tensors on
    # torch's must be done)
    torch.cuda.current_stream(dev).synchronize()
    _core.coassign_topk_many_dev(
        _cores(engines), [int(v.data_ptr()) for v in values], n_q, t_ptrs,
        n_t, k, _coassign_topk_flags(other, exclude_self),
        int(index.data_ptr()), int(prob.data_ptr()), k, single)
    return index, prob


def coassign_topk_many_torch(engines, values, other=None, k=10,
                             exclude_self=None):
    """coassign_topk_many for device tensors (one 4-byte-per-row CUDA tensor
    per feature) -> (index int32 [n, k], prob float32 [n, k]) on the same
    device; nothing is staged through the host."""
    return _coassign_topk_torch(engines, values, other, k, exclude_self,
                                False)


def _resident_range(engines, row_begin, row_end):
    """row_end None: the first engine's row count"""
    if row_end is None:
        first = engines[0] if engines else None
        row_end = 0 if first is None else first.core.row_count()
    return int(row_begin), int(row_end)


def _search_resident(engines, values, k, row_begin, row_end, single):
    row_begin, row_end = _resident_range(engines, row_begin, row_end)
    index, prob = _core.search_resident_many(
        _cores(engines), list(values), row_begin, row_end, k, 0, single)
    return index.view(np.int32), prob


def search_resident_many(engines, values, k=10, row_begin=0, row_end=None):
    """Which rows of the table are most like this record: for every row q of
    `values` (rows that are NOT in the table, one host array per feature) the
    k RESIDENT rows b of [row_begin, row_end) (None: every row) it most likely
    shares a slot with, over M engines that hold the same rows in the same
    order.  -> (index int32 [n, k], prob float32 [n, k]).
    prob = (1/M) sum_e r_e,q[slot_e(b)] with r = `responsibilities` and
    slot_e(b) the group row b has in engine e: the probability that
    `predict(mode="sample")` puts q into the slot b occupies, the engine drawn
    uniformly.  It is not normalised over b, and rows that share a group in
    every engine have bit-equal cells: with one engine the k targets are the k
    lowest-indexed rows of the best group; it takes several chains to tell
    rows apart.  Targets by prob descending, among bit-equal cells by index
    ascending; index is the row's index in the table; where the range has
    fewer than k rows the rest is index -1 and probability +0.  k is at most
    128.  A row whose logp is not finite on some engine has an unspecified
    result row.  Nothing in the engines changes."""
    return _search_resident(list(engines), values, k, row_begin, row_end,
                            False)


def _search_resident_torch(engines, values, k, row_begin, row_end, single):
    import torch
    row_begin, row_end = _resident_range(engines, row_begin, row_end)
    values = _device_columns(values)
    n_q = int(values[0].numel())
    dev = values[0].device
    k = int(k)
    index = torch.empty((n_q, k), dtype=torch.int32, device=dev)
    prob = torch.empty((n_q, k), dtype=torch.float32, device=dev)
    # (the library works on its own stream: what filled the tensors on
    # torch's must be done)
    torch.cuda.current_stream(dev).synchronize()
    _core.search_resident_many_dev(
        _cores(engines), [int(v.data_ptr()) for v in values], n_q, row_begin,
        row_end, k, 0, int(index.data_ptr()), int(prob.data_ptr()), k, single)
    return index, prob


def search_resident_many_torch(engines, values, k=10, row_begin=0,
                               row_end=None):
    """search_resident_many for device tensors (one 4-byte-per-row CUDA
    tensor per feature) -> two [n, k] tensors on the same device; nothing is
    staged through the host."""
    return _search_resident_torch(list(engines), values, k, row_begin,
                                  row_end, False)


def _coassign_resident_topk(engines, rows, k, exclude_self, row_begin,
                            row_end, single):
    row_begin, row_end = _resident_range(engines, row_begin, row_end)
    index, prob = _core.coassign_resident_topk_many(
        _cores(engines), rows, row_begin, row_end, k,
        _core.COASSIGN_EXCLUDE_SELF if exclude_self else 0, single)
    return index.view(np.int32), prob


def coassign_resident_topk_many(engines, rows, k=10, exclude_self=True,
                                row_begin=0, row_end=None):
    """Which rows of the table are most like this row of the table: for every
    index rows[a] the k RESIDENT rows b of [row_begin, row_end) (None: every
    row) that share its group in the most of the M engines -- the k largest
    cells of `coassign_resident_many(engines, rows, arange(N))`'s row a, bit
    for bit, without the [n, N] matrix.  -> (index int32 [n, k], prob float32
    [n, k]), ordered and filled as `search_resident_many`'s.  exclude_self
    leaves b == rows[a] out (the row, not the position: duplicates in `rows`
    are legal).  Nothing in the engines changes."""
    return _coassign_resident_topk(list(engines), rows, k, exclude_self,
                                   row_begin, row_end, False)


def _coassign_resident_topk_torch(engines, rows, k, exclude_self, row_begin,
                                  row_end, single):
    import torch
    row_begin, row_end = _resident_range(engines, row_begin, row_end)
    ra = _device_rows(rows)
    dev = ra.device
    n_q = int(ra.numel())
    k = int(k)
    index = torch.empty((n_q, k), dtype=torch.int32, device=dev)
    prob = torch.empty((n_q, k), dtype=torch.float32, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    _core.coassign_resident_topk_many_dev(
        _cores(engines), int(ra.data_ptr()), n_q, row_begin, row_end, k,
        _core.COASSIGN_EXCLUDE_SELF if exclude_self else 0,
        int(index.data_ptr()), int(prob.data_ptr()), k, single)
    return index, prob


def coassign_resident_topk_many_torch(engines, rows, k=10, exclude_self=True,
                                      row_begin=0, row_end=None):
    """coassign_resident_topk_many for a device index tensor -> two [n, k]
    tensors on the same device; nothing is staged through the host."""
    return _coassign_resident_topk_torch(list(engines), rows, k, exclude_self,
                                         row_begin, row_end, False)


def predict_feature_many(engines, values, target, candidates=None,
                         observed=None, mode="map", seed=0, member_seed=None,
                         draw_base=0, members=False):
    """Given some cells of rows that are NOT in the table, the cell that is
    missing, against M engines at once: feature `target`'s predictive given
    the others, averaged over the members of an ensemble (the chains of
    sweep_sequential_many, each one posterior sample).  values, candidates
    and observed are `Gibbs.predict_feature`'s.
    -> (joint [n, C], base [n], choice, member, members_joint, members_base,
    prior_totals):
    joint[q, c] = log (1/M) sum_e p(x_t = candidates[c], observed cells |
    engine e) and base[q] = log (1/M) sum_e p(observed cells | engine e): the
    in-order log_sum_exp (random.cc:78-92) over the engines of
    `Gibbs.predict_feature`'s joint and base -- under LowEntropy each minus
    that engine's prior_total first -- minus fast_log(M).
    joint - base[:, None] is the ensemble's log conditional of the target.  It
    is a RATIO OF AVERAGES, sum_e p(x_t, x_obs | e) / sum_e p(x_obs | e): the
    members' conditionals weighted by how well each member explains the
    observed cells.  It is NOT the mean of the members' joint - base, which a
    loop over predict_feature would give and which weights every member
    alike; under LowEntropy the members' unnormalised driver mass does not
    cancel in it either, each member having its own.
    choice[q] indexes the candidates: mode "sample" draws it from the folded
    joint[q] with engine step draw_base + q + 1 of `seed`, "map" takes the
    first maximum.  member[q] is the engine drawn from the members' base
    values, the posterior over the members given the observed cells, with
    engine step draw_base + q + 1 of `member_seed` (None: seed + 1), or for
    "map" the first engine of maximal value; `member`, then sample_rows on
    that engine, draws the missing cells from the ensemble.  mode None leaves
    both out.  members_joint [M, n, C] and members_base [M, n]
    (members=True) are the planes the folds ran over, prior_totals the
    engines' prior totals.  The engines share one feature list and one
    clustering model; nothing in them changes."""
    if member_seed is None:
        member_seed = seed + 1
    return _core.predict_feature_many(
        _cores(engines), list(values), target, candidates, observed,
        Gibbs._PREDICT_MODES[mode], _core.rng_seed(seed),
        _core.rng_seed(member_seed), draw_base, members)


def predict_feature_many_torch(engines, values, target, candidates=None,
                               observed=None, mode="map", seed=0,
                               member_seed=None, draw_base=0, members=False):
    """predict_feature_many for device tensors (one 4-byte-per-row CUDA tensor
    per feature, the target's may be None; observed a CUDA int32 tensor or
    None; candidates stay a host list): the results but prior_totals (numpy)
    are tensors on the same device and nothing is staged through the host.
    joint - base[:, None] is the ensemble's conditional, a ratio of averages
    and not the mean of the members' conditionals (see predict_feature_many).
    -> (joint, base, choice, member, members_joint, members_base,
    prior_totals)"""
    import torch
    if member_seed is None:
        member_seed = seed + 1
    values = [None if v is None else v.contiguous() for v in values]
    given = [v for v in values if v is not None]
    if observed is not None:
        observed = observed.contiguous()
    ref = given[0] if given else observed
    n = int(ref.numel())
    dev = ref.device
    m = Gibbs._PREDICT_MODES[mode]
    C = len(engines[0].core.feature_candidates(target, candidates))
    joint = torch.empty((n, C), dtype=torch.float32, device=dev)
    base = torch.empty(n, dtype=torch.float32, device=dev)
    choice = chosen = pj = pb = None
    if m is not None:
        choice = torch.empty(n, dtype=torch.int32, device=dev)
        chosen = torch.empty(n, dtype=torch.int32, device=dev)
    if members:
        pj = torch.empty((len(engines), n, C), dtype=torch.float32,
                         device=dev)
        pb = torch.empty((len(engines), n), dtype=torch.float32, device=dev)
    # (the library works on its own stream: what filled the tensors on
    # torch's must be done)
    torch.cuda.current_stream(dev).synchronize()
    totals = _core.predict_feature_many_dev(
        _cores(engines),
        [0 if v is None else int(v.data_ptr()) for v in values], n,
        0 if observed is None else int(observed.data_ptr()), target,
        candidates, int(joint.data_ptr()), int(base.data_ptr()),
        int(choice.data_ptr()) if choice is not None else 0,
        int(chosen.data_ptr()) if chosen is not None else 0,
        0 if m is None else m, _core.rng_seed(seed),
        _core.rng_seed(member_seed), draw_base,
        int(pj.data_ptr()) if pj is not None else 0, n * C,
        int(pb.data_ptr()) if pb is not None else 0, n, True)
    return joint, base, choice, chosen, pj, pb, totals


def marginals_many(engines, values, masks, members=False):
    """Rows that are NOT in the table: the log marginals of S feature subsets
    per row, averaged over the members of an ensemble of M engines (the
    chains of sweep_sequential_many, each one posterior sample).
    values: one host array per feature; None for a feature no mask names
    (words of such features are never read).  masks: S >= 1 uint32 shared by
    all rows, bit f set when the subset names feature f; duplicates and 0 are
    allowed; a bit beyond the feature list, or a named feature whose column is
    None, fails before any launch naming the mask's index.
    -> (logp [n, S] float32, members_logp [M, n, S] or None, prior_totals
    [M]):
    members_logp[e, q, s] = log_sum_exp over all groups of engine e, empty
    ones included, of the clustering model's score_value folded in feature
    order with the score_value of every feature in masks[s] at row q's value
    (mixture.hpp:416-425, random.cc:78-92); an unnamed feature contributes
    nothing; under LowEntropy minus that engine's prior_total.  It is
    `Gibbs.predict_feature`'s base under the row mask masks[s] (any target
    outside it), `predict`'s logp for the mask of all features and its
    prior_total for mask 0, bit for bit.
    logp[q, s] = log (1/M) sum_e p(x_q[masks[s]] | engine e): the in-order
    log_sum_exp over the engines minus fast_log(M), as `predict_many` and
    `predict_feature_many` fold theirs.  Every feature's term is evaluated
    once per (engine, row, group) and shared by the S subsets.  A named
    DirichletDiscrete value >= dim or BetaBernoulli value > 1 fails naming the
    first such row.  The engines share one feature list and one clustering
    model; nothing in them changes."""
    return _core.marginals_many(_cores(engines), list(values), masks, members)


def _marginals_torch(engines, values, masks, members, single):
    import torch
    given = [v for v in values if v is not None]
    if not given:
        raise RuntimeError("marginals_many: no column tells the number of "
                           "rows")
    # (contiguous, 4 bytes per row, one length, one CUDA device)
    checked = iter(_device_columns(given))
    values = [None if v is None else next(checked) for v in values]
    given = [v for v in values if v is not None]
    n = int(given[0].numel())
    dev = given[0].device
    masks = np.ascontiguousarray(masks, dtype=np.uint32).reshape(-1)
    S = max(len(masks), 1)
    logp = torch.empty((n, S), dtype=torch.float32, device=dev)
    planes = None
    if members:
        planes = torch.empty((len(engines), n, S), dtype=torch.float32,
                             device=dev)
    # (the library works on its own stream: what filled the tensors on
    # torch's must be done)
    torch.cuda.current_stream(dev).synchronize()
    totals = _core.marginals_many_dev(
        _cores(engines),
        [0 if v is None else int(v.data_ptr()) for v in values], n, masks,
        int(logp.data_ptr()),
        int(planes.data_ptr()) if planes is not None else 0, n * S, True,
        single)
    return logp, planes, totals


def marginals_many_torch(engines, values, masks, members=False):
    """marginals_many for device tensors (one 4-byte-per-row CUDA tensor per
    feature, None for a feature no mask names; masks stay a host list): logp
    and members_logp are tensors on the same device and nothing is staged
    through the host; prior_totals is numpy.
    -> (logp, members_logp, prior_totals)"""
    return _marginals_torch(engines, values, masks, members, False)


def relate_many(engines, n_samples, seed=0, member_seed=None, draw_base=0,
                moments=False):
    """Which columns depend on each other: the mutual information of every
    feature pair, and every feature's entropy, under the ensemble's predictive
    p = (1/M) sum_e p_e, estimated from n_samples rows drawn from it.
    -> (mi [F, F] float64, stderr [F, F] float64).
    The rows are the ones `sample_rows_many(engines, n_samples, seed=seed,
    member_seed=member_seed, draw_base=draw_base)` returns (nothing observed);
    they are scored on the device by `marginals_many` with the masks {i} and
    {i, j}, and mi[i, j] = mi[j, i] is the mean over the rows of
    d = logp_ij - logp_i - logp_j, mi[i, i] the mean of -logp_i: the entropy
    of feature i (the differential entropy of a NormalInverseChiSq feature;
    under LowEntropy the members are normalised, so it is that of a proper
    density).  stderr = sqrt(sample variance of d / n_samples), +inf for one
    row; none fails.  The moments are summed in float64 in a fixed order:
    equal calls give equal bits.  A Monte Carlo estimate of a pair's mutual
    information can be slightly negative.  A drawn row whose marginals are not
    finite makes the cells it enters NaN.  Conditional variants are composed
    from `sample_rows_many(values, observed)` and `marginals_many`.
    moments=True adds the sums themselves, [F, F, 2] float64 (sum d, sum
    d^2), which pool over calls of disjoint draw_base ranges.  Nothing in the
    engines changes."""
    if member_seed is None:
        member_seed = seed + 1
    out = _core.relate_many(_cores(engines), n_samples, _core.rng_seed(seed),
                            _core.rng_seed(member_seed), draw_base)
    return out if moments else out[:2]


def sample_rows_many(engines, n=None, values=None, observed=None, seed=0,
                     member_seed=None, draw_base=0, base=False):
    """Rows that are NOT in the table, drawn from an ensemble of M engines
    (the chains of sweep_sequential_many, each one posterior sample): per row
    a member first, then a group in that member, then the cells.  n, values
    and observed are `Gibbs.sample_rows`'s.
    -> (columns, groups, members), with base=True (columns, groups, members,
    base):
    members[q] is the engine drawn from p(engine | observed cells of row q),
    proportional to p(observed cells | engine) -- `predict_feature_many`'s
    member: the in-order fold over the engines of `Gibbs.predict_feature`'s
    base, under LowEntropy each minus that engine's prior_total -- with engine
    step draw_base + q + 1 of `member_seed` (None: seed + 1); groups[q] and
    the unobserved cells of row q are what
    engines[members[q]].sample_rows(n, values, observed, seed, draw_base)
    gives row q, the group as that engine's global id; observed cells come
    back as given.  base[q] = log (1/M) sum_e p(observed cells | engine e).
    With one engine it is that engine's sample_rows.  The engines share one
    feature list and one clustering model; nothing in them changes."""
    if member_seed is None:
        member_seed = seed + 1
    cols, groups, members, b = _core.sample_rows_many(
        _cores(engines), n, None if values is None else list(values),
        observed, _core.rng_seed(seed), _core.rng_seed(member_seed),
        draw_base)
    return (cols, groups, members, b) if base else (cols, groups, members)


def sample_rows_many_torch(engines, n=None, values=None, observed=None,
                           seed=0, member_seed=None, draw_base=0, out=None,
                           base=False):
    """sample_rows_many for device tensors (values: one 4-byte-per-row CUDA
    tensor per feature or None; observed a CUDA int32 tensor or None): the
    results are tensors on the same device (the current one when nothing is
    given) and nothing is staged through the host.  out: the tensors to fill,
    one per feature; out[f] may be values[f] itself, which completes the rows
    in place (only unobserved cells are written).
    -> (columns, groups, members), with base=True (..., base)"""
    import torch
    if member_seed is None:
        member_seed = seed + 1
    if values is not None and observed is None:
        raise RuntimeError("sample_rows_many: values need an observed mask")
    if observed is not None:
        observed = observed.contiguous()
        n = int(observed.numel())
        dev = observed.device
    else:
        values = None
        dev = torch.device("cuda", torch.cuda.current_device())
    if values is not None:
        values = [None if v is None else v.contiguous() for v in values]
    if out is None:
        out = [torch.empty(n, dtype=torch.float32
                           if s.kind == _core.KIND_NICH else torch.int32,
                           device=dev) for s in engines[0].shareds]
    groups = torch.empty(n, dtype=torch.int32, device=dev)
    members = torch.empty(n, dtype=torch.int32, device=dev)
    b = torch.empty(n, dtype=torch.float32, device=dev) if base else None
    # (the library works on its own stream: what filled the tensors on
    # torch's must be done)
    torch.cuda.current_stream(dev).synchronize()
    _core.sample_rows_many_dev(
        _cores(engines),
        None if values is None
        else [0 if v is None else int(v.data_ptr()) for v in values], n,
        0 if observed is None else int(observed.data_ptr()),
        [int(o.data_ptr()) for o in out], int(groups.data_ptr()),
        int(members.data_ptr()), int(b.data_ptr()) if base else 0,
        _core.rng_seed(seed), _core.rng_seed(member_seed), draw_base)
    return (out, groups, members, b) if base else (out, groups, members)


class ShardedGibbs(object):
    """Row-sharded Gibbs over the ranks of a torch.distributed process group.

    Every rank holds rows [row_offset, row_offset + n_local) and a full
    replica of the statistics.  A sub-sweep scores `batch_rows` local rows per
    rank against the common snapshot, turns the local moves into integer
    deltas, sums the deltas over ranks with ONE all-reduce, applies the sum
    and normalises the group set identically on every rank.  Row i always
    uses engine draw (draw_base + global index of i), so the result does not
    depend on the number of ranks for a given batch composition.

    `backend` is the per-rank compute object (a GibbsEngine-like); the
    distributed tests substitute a CPU stand-in to exercise this driver with
    gloo.
    """

    def __init__(self, backend, n_local, row_offset, group=None, device=None,
                 force_collective=False, columns=None, assign_packed=None):
        """columns: the local value columns (per feature a 4-byte-per-row
        tensor, as given to load_rows); assign_packed: the local initial
        assignment.  Both are needed only when a feature has order-dependent
        statistics (NormalInverseChiSq, GammaPoisson's log_prod): those are
        exchanged as rows, not as sums."""
        import torch.distributed as dist
        self.dist = dist
        self.backend = backend
        self.n_local = int(n_local)
        self.row_offset = int(row_offset)
        self.group = group
        self.device = device
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        # force_collective: take the delta + all-reduce path even with one
        # rank (what N > 1 runs, exercised on a single GPU)
        self.collective = self.world > 1 or (force_collective
                                             and dist.is_initialized())
        self._delta = None
        self._comm = None
        self._n_batches = {}    # batch_rows -> sub-sweeps per pass (all ranks)
        self.columns = columns
        self.assign_packed = assign_packed
        # (a property of the feature list: engines without such statistics
        # are never asked again -- the question would close an open
        # device-normalised run)
        self._has_ordered = backend.ordered_features() > 0
        self._exchange_mode()

    def _exchange_mode(self):
        """Order-dependent statistics travel as rows (every replica replays
        all of them) unless the backend keeps them as sums (float_stats = 1:
        one more all-reduce of a few doubles per group).  Asked again before
        every pass: whether the sums fit the backend's LDS pass depends on the
        group count, which grows."""
        backend = self.backend
        if not self._has_ordered:
            self.merged = self.ordered = False
            return
        self.merged = (self.collective
                       and getattr(backend, "float_delta_words",
                                   lambda: 0)() > 0)
        self.ordered = self.collective and not self.merged
        if self.ordered and self.columns is None:
            raise ValueError("features with order-dependent statistics need "
                             "the local value columns (columns=...)")

    def _gather_rows(self, arrays, n_pad):
        """arrays: list of (tensor-or-None, n valid) with 4-byte elements ->
        per array the concatenation over ranks (rank order) of the tensors
        padded to n_pad with 0xFFFFFFFF; ONE all-gather."""
        import torch
        pack = torch.full((len(arrays), n_pad), -1, dtype=torch.int32,
                          device=self.device)
        for i, t in enumerate(arrays):
            if t is not None and t.numel():
                pack[i, :t.numel()] = t.view(torch.int32)
        if self.world == 1:
            return [pack[i] for i in range(len(arrays))]
        if self._stage_through_host(pack):
            host = pack.cpu()
            parts = [torch.empty_like(host) for _ in range(self.world)]
            self.dist.all_gather(parts, host, group=self.group)
            out = torch.stack(parts).to(pack.device)
        else:
            out = torch.empty((self.world,) + tuple(pack.shape),
                              dtype=torch.int32, device=self.device)
            self.dist.all_gather(list(out.unbind(0)), pack, group=self.group)
        return [out[:, i, :].reshape(-1).contiguous()
                for i in range(len(arrays))]

    def _replay(self, old, new, cols, n_pad, reset):
        """cols: per feature the local slice (or None)"""
        arrays = [new] + ([old] if old is not None else []) + [
            c for c in cols if c is not None]
        got = self._gather_rows(arrays, n_pad)
        new_all = got[0]
        old_all = got[1] if old is not None else None
        rest = got[2:] if old is not None else got[1:]
        ptrs, j = [], 0
        for c in cols:
            if c is None:
                ptrs.append(0)
            else:
                ptrs.append(int(rest[j].data_ptr()))
                j += 1
        self.backend.replay_ordered_dev(
            int(old_all.data_ptr()) if old_all is not None else 0,
            int(new_all.data_ptr()), ptrs, int(new_all.numel()), bool(reset))

    def _is_ordered(self, f):
        return self.backend.feature_is_ordered(f)

    def _stage_through_host(self, tensor):
        """device tensors under a host-only backend (gloo): the multi-rank
        tests on a single GPU run the real engine this way"""
        return tensor.is_cuda and self.dist.get_backend(self.group) == "gloo"

    def _all_reduce(self, tensor, op=None):
        if not self.collective:
            return
        op = op if op is not None else self.dist.ReduceOp.SUM
        if self._stage_through_host(tensor):
            host = tensor.cpu()
            self.dist.all_reduce(host, op=op, group=self.group)
            tensor.copy_(host)
        else:
            self.dist.all_reduce(tensor, op=op, group=self.group)

    def sync_initial_stats(self):
        """After every rank loaded ITS rows: make the statistics global."""
        import torch
        if not self.collective:
            return
        n = self.backend.stat_words()
        t = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.backend.export_stats_dev(int(t.data_ptr()))
        if self.merged:   # (from the rank's OWN statistics: before the import)
            words = self.backend.float_delta_words()
            image = torch.zeros(words, dtype=torch.float64, device=self.device)
            self.backend.export_float_moments_dev(int(image.data_ptr()))
        self._all_reduce(t)
        self.backend.import_stats_dev(int(t.data_ptr()))
        if self.merged:
            self._all_reduce(image)
            self.backend.import_float_moments_dev(int(image.data_ptr()))
        if self.ordered:
            # order-dependent statistics: every replica replays ALL rows in
            # global order (Group::add_value per row, in row order)
            if self.assign_packed is None:
                raise ValueError("sync_initial_stats needs assign_packed")
            nmax = torch.tensor([self.n_local], dtype=torch.int64,
                                device=self.device)
            self._all_reduce(nmax, op=self.dist.ReduceOp.MAX)
            cols = [c if self._is_ordered(f) else None
                    for f, c in enumerate(self.columns)]
            self._replay(None, self.assign_packed, cols, int(nmax.item()),
                         reset=True)

    def use_native_comm(self, comm=None, transport=None):
        """Give the library its own communicator (or share `comm`, the
        `native_comm` of another engine of this process group): the sub-sweep
        loop then runs inside it, the all-reduce on the engine's stream (no
        Python and no stream hop per sub-sweep).  Collective.  transport:
        "rccl" (the default under an NCCL process group) or "host" -- the
        library's shared-memory transport for ranks that share one GPU (the
        default under gloo with device tensors: RCCL refuses two ranks on a
        device).  Returns False -- and the torch.distributed path stays in use
        -- when the engine has order-dependent statistics or the transport
        cannot be had."""
        import torch
        core = self.backend
        if not (self.collective and not self.ordered
                and hasattr(core, "sweep_sharded")):
            return False
        backend = self.dist.get_backend(self.group)
        if transport is None:
            transport = "rccl" if backend == "nccl" else "host"
        if transport == "rccl" and backend != "nccl":
            return False
        from . import _core
        if comm is not None:
            self._comm = comm
            return True
        # (flags and the id travel on whatever the process group moves:
        # device tensors under NCCL, host tensors under gloo)
        where = self.device if backend == "nccl" else "cpu"
        have = transport == "host" or _core.comm_available()
        ok = torch.tensor([1 if have else 0], dtype=torch.int32, device=where)
        self.dist.all_reduce(ok, op=self.dist.ReduceOp.MIN, group=self.group)
        if not int(ok.item()):
            return False
        rank = self.dist.get_rank(self.group)
        uid = torch.zeros(128, dtype=torch.uint8, device=where)
        if rank == 0:
            make = (_core.comm_unique_id_host if transport == "host"
                    else _core.comm_unique_id)
            uid.copy_(torch.from_numpy(make()))
        self.dist.broadcast(uid, src=self.dist.get_global_rank(
            self.group, 0) if self.group is not None else 0, group=self.group)
        try:
            comm = _core.Comm(uid.cpu().numpy(), rank, self.world)
        except RuntimeError:
            comm = None
        ok.fill_(0 if comm is None else 1)   # all ranks or none
        self.dist.all_reduce(ok, op=self.dist.ReduceOp.MIN, group=self.group)
        if not int(ok.item()):
            return False
        self._comm = comm
        return True

    def partition_by_value(self):
        """Collective, with a native communicator, after sync_initial_stats:
        the rows are placed so that no value of the (one, categorical)
        feature has rows on two ranks -- checked -- and the sub-sweeps
        exchange 3 words per group instead of the cells."""
        if self._comm is None:
            raise RuntimeError("partition_by_value needs use_native_comm()")
        self.backend.partition_by_value(self._comm)
        self._partitioned = True

    def gather_cells(self):
        """Collective: the replicas of value-partitioned ranks are whole again
        (before groups are read, validated, exported)."""
        self.backend.gather_cells(self._comm)

    @property
    def native_comm(self):
        return self._comm

    # -- hyper-parameters: every rank calls these alike.  The scoring ones
    # read every cell, so value-partitioned ranks gather theirs first; with
    # equal rng_state the replicas choose the same index, because their
    # statistics are equal.
    def _whole(self):
        if self._comm is not None and getattr(self, "_partitioned", False):
            self.backend.gather_cells(self._comm)

    def predict(self, values, mode="sample", seed_state=0, draw_base=0):
        """Each rank predicts ITS queries against the common state (as
        Gibbs.predict; seed_state is a raw engine state, as sweep's).  A
        value-partitioned rank gathers its cells first."""
        self._whole()
        return self.backend.predict(list(values), Gibbs._PREDICT_MODES[mode],
                                    seed_state, draw_base)

    def predict_feature(self, values, target, candidates=None, observed=None,
                        mode="map", seed_state=0, draw_base=0, staged=True):
        """Each rank asks for ITS queries' missing cell against the common
        state (as Gibbs.predict_feature; seed_state is a raw engine state).
        A value-partitioned rank gathers its cells first."""
        self._whole()
        return self.backend.predict_feature(
            list(values), target, candidates, observed,
            Gibbs._PREDICT_MODES[mode], seed_state, draw_base,
            0 if staged else _core.PREDICT_FEATURE_RECOMPUTE)

    def sample_rows(self, n=None, values=None, observed=None, seed_state=0,
                    draw_base=0):
        """Each rank draws ITS rows from the common state (as
        Gibbs.sample_rows; seed_state is a raw engine state).  Cell (q, f)
        and row q's group depend on (seed_state, draw_base + q) alone, so
        ranks that share a seed_state MUST be given disjoint
        [draw_base, draw_base + n) ranges, or they draw the same rows.  A
        value-partitioned rank gathers its cells first."""
        self._whole()
        return self.backend.sample_rows(n, None if values is None
                                        else list(values), observed,
                                        seed_state, draw_base)

    def score_data(self):
        self._whole()
        return self.backend.score_data()

    def score_data_grid(self, feature, shareds):
        self._whole()
        return self.backend.score_data_grid(feature, list(shareds))

    def score_counts_grid(self, alphas, ds):
        return self.backend.score_counts_grid(alphas, ds)

    def set_shared(self, feature, shared):
        self.backend.set_shared(feature, shared)

    def set_clustering(self, alpha, d):
        self.backend.set_clustering(alpha, d)

    def sample_hypers(self, feature, shareds, rng_state):
        self._whole()
        return self.backend.sample_hypers(feature, list(shareds), rng_state)

    def sample_hypers_pass(self, feature, grids, rng_state, coords=None):
        """Every rank calls it alike: the chains are summed in a fixed order,
        so replicas with equal rng_state choose alike.  A value-partitioned
        rank gathers its cells first."""
        self._whole()
        return self.backend.sample_hypers_pass(feature, grids, rng_state,
                                               coords)

    def sample_clustering(self, alphas, ds, rng_state):
        return self.backend.sample_clustering(alphas, ds, rng_state)

    def sweep(self, batch_rows, seed_state, draw_base=0):
        """One pass over the local shard; all ranks take the same number of
        sub-sweeps (shards are equal up to one batch of padding)."""
        import torch
        self._exchange_mode()
        if self.ordered:
            self._comm = None   # (rows, not sums: the Python loop below)
        n_batches = (self.n_local + batch_rows - 1) // batch_rows
        if self.collective:
            if self._n_batches.get(batch_rows) is None:
                nb = torch.tensor([n_batches], dtype=torch.int64,
                                  device=self.device)
                self._all_reduce(nb, op=self.dist.ReduceOp.MAX)
                self._n_batches[batch_rows] = int(nb.item())
            n_batches = self._n_batches[batch_rows]
        if self._comm is not None:
            # (the library's loop; whether the group set is normalised on the
            # device is agreed among the ranks inside it, when a run opens)
            self.backend.sweep_sharded(self._comm, n_batches, batch_rows,
                                       seed_state, draw_base)
            return
        if not self.collective and hasattr(self.backend, "sweep"):
            # one rank, no exchange: the library's own loop (which queues the
            # whole pass without a host round trip where it can)
            self.backend.sweep(0, self.n_local, batch_rows, seed_state,
                               draw_base)
            return
        for b in range(n_batches):
            r0 = min(self.n_local, b * batch_rows)
            r1 = min(self.n_local, r0 + batch_rows)
            self.backend.batch_sample(r0, r1, seed_state, draw_base)
            if not self.collective:
                self.backend.batch_apply_local()
            else:
                n = self.backend.stat_words()
                if self._delta is None or self._delta.numel() < n:
                    # headroom: the image grows with the group count
                    self._delta = torch.empty(n + n // 4 + 1024,
                                              dtype=torch.int32,
                                              device=self.device)
                delta = self._delta[:n]
                self.backend.batch_delta_dev(int(delta.data_ptr()))
                self._all_reduce(delta)
                self.backend.batch_apply_delta_dev(int(delta.data_ptr()))
                if self.merged:
                    words = self.backend.float_delta_words()
                    fd = torch.empty(words, dtype=torch.float64,
                                     device=self.device)
                    self.backend.batch_float_delta_dev(int(fd.data_ptr()))
                    self._all_reduce(fd)
                    self.backend.batch_apply_float_delta_dev(
                        int(fd.data_ptr()))
                if self.ordered:
                    nb_rows = r1 - r0
                    old = torch.empty(nb_rows, dtype=torch.int32,
                                      device=self.device)
                    new = torch.empty(nb_rows, dtype=torch.int32,
                                      device=self.device)
                    self.backend.batch_moves_dev(int(old.data_ptr()),
                                                 int(new.data_ptr()))
                    cols = [c[r0:r1] if self._is_ordered(f) else None
                            for f, c in enumerate(self.columns)]
                    self._replay(old, new, cols, batch_rows, reset=False)
            self.backend.batch_finish()
