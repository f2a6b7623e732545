"""The engine's and the stand-alone mixture's log marginal likelihoods held to
float64 closed forms (tests/f64_marginals.py): Gibbs.score_data,
score_data_grid and score_counts_grid (k_hyper_dd_chains, k_hyper_dd_close,
k_hyper_py_grid, k_score_data_terms, k_score_data_serial, k_score_data_grid),
_core.SlaveMixture.score_data / score_data_grid built from the engine's groups
(k_score_data_dd, k_score_data_grid) and _core.py_score_counts
(k_py_score_counts).

The float64 side is rebuilt from gpu.assignments(), the columns and the
assignments recorded after every sweep; nothing of it comes from the engine's
or the oracle's statistics.  Where the oracle promises equality the scores
are also compared bit for bit with the oracle beside the engine, so that a
failure says which side moved.  The shapes are those of
tests/test_f64_marginals.py, where the planted bugs are shown to leave the
band at them."""
import numpy as np
import pytest

import f64_marginals as fm
import f64_scores as fx
import oracle_lib as ol
import workloads
from test_f64_marginals import (MEASURED, SHAPES, check_grid_posterior,
                                every_grid, every_py_grid, oracle_score_counts,
                                oracle_scores, ratio, report, seeds_of,
                                shape_inputs)
from test_gpu_hypers import mixture_from_groups
from test_gpu_scores_f64 import bits_equal, both

pytestmark = pytest.mark.gpu

# the engine's shapes: SHAPES, and DD-16 again on the general-rows path
ENGINE_SHAPES = {name: (spec, {}) for name, spec in SHAPES.items()}
ENGINE_SHAPES["dd16_k6_general"] = (SHAPES["dd16_k6"], {"value_sorted": 0})


def swept_engine(spec, opts, oracle_sweeps=True):
    """the engine after the shape's sweeps, the oracle beside it, and the
    float64 state rebuilt from the engine's assignments and their history"""
    config, dim, n, k, empty, alpha, d, sweeps, batch = spec
    osh, gsh, vals, assign = shape_inputs(spec)
    orc, gpu = both(osh, gsh, vals, assign, k, empty, alpha, d, opts=opts)
    history = [np.array(gpu.assignments())]
    seed = seeds_of(spec)[1]
    st_seed = ol.oracle().orc_rng_seed(seed)
    for s in range(sweeps):
        gpu.sweep(0, n, batch, seed, draw_base=s * n)
        history.append(np.array(gpu.assignments()))
        if oracle_sweeps:
            for b in range(0, n, batch):
                orc.gibbs_batch(b, min(n, b + batch), st_seed, s * n)
            assert np.array_equal(history[-1], orc.assign), s
    if not oracle_sweeps:
        # (the large states: the oracle takes the engine's state over, and
        # is there for the bit-for-bit comparison alone)
        orc.adopt(gpu, vals)
    p2g = [gpu.core.packed_to_global(i) for i in range(len(gpu))]
    prior = ("py", float(np.float32(alpha)), float(np.float32(d)))
    st = fx.State(vals, osh, history[-1], p2g, prior, history)
    assert np.array_equal(st.counts, gpu.counts())
    return orc, gpu, gsh, st, fm.Marginals(st, history)


def engine_checks(name, orc, gpu, gsh, st, mar, measure=False):
    """score_data, every grid and score_counts of one engine against the
    float64 band; -> the lines `report` printed"""
    lines, mixes = [], {}
    data, clustering = gpu.score_data()
    for fi, gname, cands, chosen in every_grid(orc, mar):
        kind = st.feats[fi].kind
        want, feats = oracle_scores(orc, mar, fi, cands, st.feats[fi])
        what = "%s f%d %s K=%d" % (name, fi, gname, st.K)
        if fi not in mixes:
            mixes[fi] = mixture_from_groups(gpu, fi, gsh[fi])
        mix = mixes[fi]
        if cands is None:
            got = np.array([data[fi]], np.float32)
            alone = np.array([mix.score_data()], np.float32)
        else:
            got = gpu.score_data_grid(fi, [c[1] for c in cands])
            alone = mix.score_data_grid([c[1] for c in cands])
        assert got.dtype == np.float32 and got.shape == want.shape
        v, band = mar.data(fi, feats, total="f64")
        w, w_alone = ratio(got, v, band), ratio(alone, v, band)
        print("%s: band %.3g, excursion / band: engine %.3f, mixture %.3f" % (
            what, float(band.max()), w, w_alone))
        if measure and cands is not None:
            lines.append(report("engine " + what, got, v, band))
        assert w <= 1.0, what
        assert w_alone <= 1.0, what + " (SlaveMixture)"
        if not len(st.assign):
            assert np.all(np.abs(got) <= band) and np.all(
                np.abs(alone) <= band)
        check_grid_posterior(got, v, band, what, chosen)
        check_grid_posterior(alone, v, band, what + " (SlaveMixture)", chosen)
        if kind != fx.DPD:
            assert bits_equal(got, want), what + ": engine != oracle"
            assert bits_equal(alone, want), what + ": SlaveMixture != oracle"
    from distributions_amd import _core
    counts = np.ascontiguousarray(gpu.counts(), np.int32)
    for gname, alphas, ds, chosen in every_py_grid(st, mar):
        got = gpu.score_counts_grid(alphas, ds)
        assert got.dtype == np.float32
        single = np.array([_core.py_score_counts(float(a), float(d), counts)
                           for a, d in zip(alphas, ds)], np.float32)
        v, band = mar.counts(alphas, ds)
        what = "%s score_counts %s K=%d" % (name, gname, st.K)
        w, w_single = ratio(got, v, band), ratio(single, v, band)
        print("%s: band %.3g, excursion / band: grid %.3f, "
              "py_score_counts %.3f" % (what, float(band.max()), w, w_single))
        if measure:
            lines.append(report("engine " + what, got, v, band))
            report("oracle " + what, oracle_score_counts(orc, st, alphas, ds),
                   v, band)
        assert w <= 1.0 and w_single <= 1.0, what
        check_grid_posterior(got, v, band, what, chosen)
    v, band = mar.counts([st.prior[1]], [st.prior[2]])
    assert abs(float(clustering) - v[0]) <= band[0], (name, clustering, v)
    return lines


@pytest.mark.parametrize("name", list(ENGINE_SHAPES))
def test_engine_marginals_are_in_the_float64_band(name):
    spec, opts = ENGINE_SHAPES[name]
    orc, gpu, gsh, st, mar = swept_engine(spec, opts)
    K = len(gpu)
    empty = np.nonzero(st.counts == 0)[0]
    if opts:
        vs, generic = gpu.path_counts()
        assert vs == 0 and generic > 0
    if name.startswith("dd256_k300"):
        # several k_hyper_dd_chains blocks, the last one partly filled
        assert K >= 300 and (st.feats[0].dim + 1) % 64 != 0
    if name == "dd256_k300":
        # empty slots inside the range, which the chains skip
        assert (empty < mar.live.max()).sum() >= 2, empty
    if name == "gp_nich_k300":
        # k_score_data_terms over two blocks, k_score_data_serial with a
        # partly filled last round of 64, k_hyper_py_grid past its 256 lanes
        assert K > 256 and (4 * K) % 64 != 0
    engine_checks(name, orc, gpu, gsh, st, mar)
    gpu.validate()


def test_every_group_empty():
    """rows loaded without a group: every score within its zero-width or
    one-rounding band of 0"""
    from distributions_amd import engine
    osh, gsh, vals, _ = workloads.make("dd_bb_gp", 100, 1)
    osh2, gsh2, vals2, _ = workloads.make("nich", 100, 1)
    osh3, gsh3, vals3, _ = workloads.make("dpd_other", 100, 1)
    osh, gsh, vals = osh + osh2 + osh3, gsh + gsh2 + gsh3, vals + vals2 + vals3
    gpu = engine.Gibbs(1.0, 0.2, gsh)
    gpu.load_rows_unassigned(vals, 3)
    orc = ol.OracleMixture(1.0, 0.2, osh)
    orc.init_empty(vals, 3)
    assert len(gpu) == 3 and not gpu.counts().any()
    p2g = [gpu.core.packed_to_global(i) for i in range(len(gpu))]
    st = fx.State([v[:0] for v in vals], osh, np.zeros(0, np.int64), p2g,
                  ("py", 1.0, float(np.float32(0.2))))
    engine_checks("all_empty", orc, gpu, gsh, st, fm.Marginals(st))


@pytest.mark.parametrize("name", list(MEASURED))
def test_large_state_sanity_band_and_measurement(name):
    """the states DESIGN.md 4.8 reports on: the derived band is some tens of
    nats there and proves little, so it is a sanity bound; the excursions,
    their spread over a grid and the total variation between the two
    softmaxes are printed, the engine's beside the oracle's (equal for
    DirichletDiscrete and the scalar kinds, whose scores are the same
    bits)"""
    orc, gpu, gsh, st, mar = swept_engine(MEASURED[name], {},
                                          oracle_sweeps=False)
    assert len(mar.live) > 1000
    for line in engine_checks(name, orc, gpu, gsh, st, mar, measure=True):
        assert line
