"""The float64 sampling reference (tests/f64_sampling.py) against the oracle's
batched sampler, and the proof that its per-row check has power where the
agreement rate of the scan tests has none.

Every draw of orc_mix_batch_sample must lie in the accepted set of the exact
band.  Then re-implementations of the same sampler with a planted bug each
fail that check while passing the 99.5 % agreement rule
(tests/test_gpu_scan.py) -- the gap the per-row check closes."""
import ctypes

import numpy as np
import pytest

import f64_sampling as fs
import oracle_lib as ol
import workloads


def test_uniforms_are_the_oracles():
    L = ol.oracle()
    seed, base = 987654321, 12345
    rows = np.r_[0:300, 4095, 4096, 1 << 20, (1 << 31) + 7]
    want = []
    for r in rows:
        st = ctypes.c_uint32(L.orc_rng_jump(L.orc_rng_seed(seed), base + r))
        want.append(L.orc_sample_unif01(ctypes.byref(st)))
    got = fs.uniforms(seed, base, rows)
    assert np.array_equal(got.view(np.uint32),
                          np.array(want, np.float32).view(np.uint32))


def test_fast_exp_table_bounds_the_host_fast_exp():
    """FAST_EXP_REL re-measured on a stride of the binary32 values it covers
    (the committed table came from all of them)"""
    L = ol.oracle()
    lo = int(np.float32(2.0 ** -30).view(np.uint32))
    hi = int(np.float32(87.0).view(np.uint32))
    x = (np.arange(lo, hi, 97, dtype=np.uint32)
         | np.uint32(0x80000000)).view(np.float32)
    y = np.zeros_like(x)
    L.orc_vec_fast_exp(x.size, x, y)
    rel = np.abs(y.astype(np.float64) / np.exp(x.astype(np.float64)) - 1)
    b = np.floor(-x.astype(np.float64)).astype(int)
    assert (rel <= fs.FAST_EXP_REL[b]).all()


# ---------------------------------------------------------------------------
# the oracle's batched draws


def oracle_case(config, n, k, alpha=1.0, d=0.2, dim=None, seed=workloads.SEED,
                assign=None, vals_osh=None):
    if vals_osh is None:
        osh, _, vals, assign0 = workloads.make(config, n, k, seed=seed,
                                               dim=dim)
    else:
        vals, osh = vals_osh
        assign0 = None
    assign = assign0 if assign is None else assign
    orc = ol.OracleMixture(alpha, d, osh)
    orc.init_from_assignments(vals, assign, k, 1)
    return orc


class Batch(object):
    """one batch [0, n) of the oracle: slots before and after, per row its
    batch-semantics scores and uniform"""

    def __init__(self, orc, seed=777, draw_base=0):
        self.orc = orc
        n = orc.n_rows
        self.K = K = len(orc)
        self.p2g = np.array([orc.packed_to_global(i) for i in range(K)])
        counts = orc.counts()
        be = ol.OracleBackend(orc, 0)
        g = np.array([orc.L.orc_mix_global_to_packed(orc.h, int(a))
                      for a in orc.assign], np.int64)
        self.g = g
        self.kl = np.where(counts[g] == 1, K - 1, K)
        be.batch_sample(0, n, ol.oracle().orc_rng_seed(seed), draw_base)
        _, _, old, new, _ = be._open
        be.batch_finish()
        assert np.array_equal(old[:n], g)
        new = new[:n].astype(np.int64)
        # back from ids to the slot of the row's score vector
        self.slot = np.where((self.kl != K) & (new == K - 1), g, new)
        self.n = n
        self.u = fs.uniforms(seed, draw_base, np.arange(n))
        self._scores = None
        # the empty slot of each row
        self.empty = np.where(self.kl != K, g,
                              np.nonzero(counts == 0)[0][0])

    def score_rows(self, rows):
        """[len(rows), K] batch-semantics scores, -inf beyond each Kl"""
        out = np.full((len(rows), self.K), -np.inf, np.float32)
        for j, r in enumerate(rows):
            s = self.orc.row_scores(int(r), int(self.g[r]))
            out[j, :len(s)] = s
        return out

    @property
    def scores(self):
        """all rows at once (the planted-bug samplers' small case only)"""
        if self._scores is None:
            self._scores = self.score_rows(np.arange(self.n))
        return self._scores

    def rows(self, sel):
        idx = np.arange(self.n)[sel]
        return fs.Rows(self.score_rows(idx), self.kl[sel], self.u[sel])


def check(batch, drawn, name, band=fs.band_exact, chunk=None):
    n, K = batch.n, batch.K
    chunk = chunk or max(64, (1 << 21) // K)   # (rows scored chunk by chunk)
    rep = fs.Report(name)
    for i0 in range(0, n, chunk):
        sel = slice(i0, i0 + chunk)
        rr = batch.rows(sel)
        rep.add(rr, band(rr), drawn[sel], np.arange(n)[sel])
    print(rep.line())
    return rep


@pytest.mark.parametrize("config,n,k,dim", [
    ("dd", 20000, 64, 256), ("dd", 20000, 1024, 256), ("dd", 32768, 8192, 256),
    ("gp_nich", 20000, 64, None), ("gp_nich", 20000, 1024, None),
    ("dpd", 20000, 1024, 1000), ("dpd", 32768, 8192, 10000),
    # half of the groups hold one row: rows alone in their group
    ("dd", 1536, 1024, 256), ("gp_nich", 96, 64, None),
    ("dpd", 12288, 8192, 1000),
])
def test_oracle_draws_are_in_the_exact_band(config, n, k, dim):
    b = Batch(oracle_case(config, n, k, dim=dim))
    rep = check(b, b.slot, "oracle %s K=%d" % (config, k + 1))
    crude = check(b, b.slot, "  (crude band)", band=fs.band_crude)
    assert rep.bad == 0, rep.line()
    assert (b.kl != b.K).any() == (n < 2 * k)
    # the derived band is never looser than the crude one here
    assert rep.inband <= crude.inband


# ---------------------------------------------------------------------------
# planted bugs


def sample_f32(batch, l_override=None, t_shift=None, u=None):
    """orc_sample_from_scores_u restated in numpy float32 (the same
    operations in the same order: bit-identical, checked below), with hooks
    for the planted bugs."""
    s = batch.scores
    n, K = s.shape
    m = s.max(1)
    l = np.zeros((n, K), np.float32)
    d = (s - m[:, None]).astype(np.float32)
    valid = np.isfinite(s)
    flat = np.ascontiguousarray(np.where(valid, d, 0).ravel(), np.float32)
    out = np.zeros_like(flat)
    ol.oracle().orc_vec_fast_exp(flat.size, flat, out)
    l = np.where(valid, out.reshape(n, K), np.float32(0))
    if l_override is not None:
        l = l_override(l)
    total = np.cumsum(l, 1, dtype=np.float32)[np.arange(n), batch.kl - 1]
    uu = batch.u if u is None else u
    t = (total * uu).astype(np.float32)
    acc = np.concatenate([t[:, None], l], 1)
    tk = np.subtract.accumulate(acc, 1, dtype=np.float32)[:, 1:]
    if t_shift is not None:
        tk = t_shift(tk, t)
    hit = (tk <= 0) & valid
    k = np.where(hit.any(1), hit.argmax(1), batch.kl - 1)
    return k


def tab_likelihoods(batch):
    """l of slot g as k_vs_scan_prepare tabulates it: the score of the row's
    value with the row still in its group (MixtureDriver::score_value +
    the slaves', then the batch shift), through the same fast_exp"""
    orc = batch.orc
    n, K = batch.scores.shape
    shift_fix = (np.float32(np.log(orc.n_rows + orc_alpha(orc)))
                 - np.float32(np.log(orc.n_rows - 1 + orc_alpha(orc))))
    out = np.zeros(n, np.float32)
    sc = np.zeros(K, np.float32)
    for r in range(n):
        orc.L.orc_mix_driver_score_value(orc.h, sc)
        for f in range(orc.F):
            orc.L.orc_mix_slave_score_value(orc.h, f, int(orc.values[f][r]),
                                            sc)
        out[r] = sc[batch.g[r]] + shift_fix
    m = batch.scores.max(1)
    x = np.ascontiguousarray(np.minimum(out - m, 0), np.float32)
    y = np.zeros_like(x)
    ol.oracle().orc_vec_fast_exp(n, x, y)
    return y


def orc_alpha(orc):
    return orc._alpha


def planted_case(alpha):
    """a planted mixture with two discrete features and one real one, rows
    in their true cluster: draws concentrated enough that a bug touching the
    new-group slot, the own slot or the last slot moves fewer than 0.5 % of
    them"""
    z, osh, _, vals = workloads.planted(12000, k_true=32, seed=3, n_cat=2,
                                        n_real=1)
    orc = ol.OracleMixture(alpha, 0.1, osh)
    orc._alpha = alpha
    orc.init_from_assignments(vals, z.astype(np.uint32), 32, 1)
    return orc


# bug -> whether it stays under the agreement rule's 0.5 % in this case (the
# two that do not move several % of the rows here; the per-row check must
# catch every one of them regardless)
BUGS = {"never_empty": True, "own_slot_gt": True, "last_unreachable": True,
        "own_slot_next": False, "neighbour_u": False}


@pytest.fixture(scope="module")
def planted_batches():
    # (3 of its 12 000 rows start a group)
    b = Batch(planted_case(1.0), seed=31337)
    b.l_tab = tab_likelihoods(b)
    return [b]


def planted(batch, bug):
    n, K = batch.scores.shape
    r = np.arange(n)
    own = batch.kl == K          # (rows alone in their group have no own slot)
    if bug == "never_empty":
        def lo(l):
            l = l.copy()
            l[r, batch.empty] = 0
            return l
        return sample_f32(batch, l_override=lo)
    if bug in ("own_slot_gt", "own_slot_next"):
        # the value-sorted scan's own-slot correction, C[k] + (k >= g ?
        # l_own - l_g : 0): `>` for `>=` leaves slot g's own comparison on
        # the tabulated l_g; "from slot g + 1" takes l_g from the next slot
        g = batch.g
        if bug == "own_slot_gt":
            def ts(tk, t):
                tk = tk.copy()
                prev = np.where(g > 0, tk[r, np.maximum(g - 1, 0)], t)
                alt = (prev - batch.l_tab).astype(np.float32)
                tk[r[own], g[own]] = alt[own]
                return tk
            return sample_f32(batch, t_shift=ts)

        def lo(l):
            l = l.copy()
            nxt = np.minimum(g + 1, batch.kl - 1)
            # delta = l_own - l_{g+1}: the prefixes hold l_g (tabulated)
            l[r[own], g[own]] = (batch.l_tab - l[r, nxt] + l[r, g])[own]
            l[r[own], g[own]] = np.maximum(l[r[own], g[own]], 0)
            return l
        return sample_f32(batch, l_override=lo)
    if bug == "last_unreachable":
        k = sample_f32(batch)
        return np.where(k == batch.kl - 1, batch.kl - 2, k)
    if bug == "neighbour_u":
        return sample_f32(batch, u=np.roll(batch.u, -1))
    raise ValueError(bug)


def test_float32_restatement_is_the_oracles(planted_batches):
    for b in planted_batches:
        assert np.array_equal(sample_f32(b), b.slot)


@pytest.mark.parametrize("bug", BUGS)
def test_planted_bug_fails_the_row_check_but_passes_the_agreement_rule(
        planted_batches, bug):
    caught = 0
    for b in planted_batches:
        drawn = planted(b, bug)
        agree = float((drawn == b.slot).mean())
        rep = check(b, drawn, "planted %s (alpha %s): agreement %.4f %%"
                    % (bug, b.orc._alpha, 100 * agree))
        if BUGS[bug]:
            assert agree > 0.995, (bug, agree)
        caught += rep.bad
        ok = check(b, b.slot, "  the unplanted sampler")
        assert ok.bad == 0
    assert caught > 0, bug
