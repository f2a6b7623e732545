"""Feature lists of four to eight features for the parity tests of the
general-row kernels (tests/test_gpu_wide_rows.py): identical bytes for the
oracle and the GPU, hyper-parameters distinct per feature so that two features
of one kind cannot be swapped unnoticed.

Columns: GPs  = Poisson(3) clipped to 15, 15 present: a table of 16 values;
         GPbig = Poisson(3) with about 40 cells in [300, 100 000]: a table of
                 64 values, those rows are handed to the wave-per-row kernel;
         BNBs = BetaNegativeBinomial values clipped to 7, 7 present: 8 values.

EXPECT: what launch_rows_scratch makes of each list with "debug.rows_fold" = 2
and batches of 3000 rows (folding goes on while J * nv <= 3000 and stops at
the first NormalInverseChiSq) -- (ops folded, instance, rows handed over).
Instances: 0 generic, 1 GN, 2 N, 3 NN, 4 G, 5 C."""
import functools

import numpy as np

import oracle_lib as ol
import workloads
from distributions_amd import engine

SEED = 20250117

#             name: (folded, instance, hands rows over)   what remains
EXPECT = {
    "mixed5": (4, 2, False),        # N
    "mixed5_big": (3, 1, True),     # G N
    "planted6": (2, 0, False),      # C C N N: generic, four ops
    "cats8": (7, 5, False),         # C
    "all_folded4": (4, 0, False),   # nothing: generic, no op
    "wide8": (5, 0, True),          # G N G: generic, three ops
    "real_first": (0, 0, False),    # N C G N G: generic, five ops
    "reals4": (0, 0, False),        # N N N N: generic, four ops
    "cats_reals": (2, 3, False),    # N N
    "cats_gp": (2, 4, True),        # G
}
NAMES = list(EXPECT)

LISTS = {
    "mixed5": ["dd16", "dd4", "bb", "gps", "nich"],
    "mixed5_big": ["dd16", "dd4", "bb", "gpbig", "nich"],
    "cats8": ["dd3"] * 8,
    "all_folded4": ["dd4", "bb", "dd8", "bb"],
    "wide8": ["dd3"] * 4 + ["bb", "gpbig", "nich", "bnbs"],
    "real_first": ["nich", "dd8", "gps", "nich", "bb"],
    "reals4": ["nich"] * 4,
    "cats_reals": ["dd16", "dd16", "nich", "nich"],
    "cats_gp": ["dd16", "dd16", "gpbig"],
    "defaults5": ["dd4", "bb", "dd8", "gps", "nich"],
}


def _spread(rng, n, count):
    """count positions, one in each of count equal stretches of the rows"""
    count = min(count, n)
    width = n // count
    return np.arange(count) * width + rng.integers(0, width, count)


def _shared(kind, i, dim=None):
    """feature i's hyper-parameters: a function of i, so distinct per feature
    -> (oracle shared, engine shared)"""
    if kind == "dd":
        alphas = [0.3 + 0.1 * i + 0.05 * ((j * (i + 2)) % dim)
                  for j in range(dim)]
        return ol.make_shared(ol.DD, alphas=alphas), engine.dd_shared(alphas)
    if kind == "bb":
        a, b = 0.4 + 0.3 * i, 2.5 - 0.2 * i
        return ol.make_shared(ol.BB, alpha=a, beta=b), engine.bb_shared(a, b)
    if kind == "gp":
        a, ib = 0.7 + 0.4 * i, 0.6 + 0.25 * i
        return (ol.make_shared(ol.GP, alpha=a, inv_beta=ib),
                engine.gp_shared(a, ib))
    if kind == "bnb":
        a, b, r = 0.8 + 0.2 * i, 0.5 + 0.15 * i, 1 + i % 3
        return (ol.make_shared(ol.BNB, alpha=a, beta=b, r=r),
                engine.bnb_shared(a, b, r))
    p = [0.3 * i - 0.5, 0.4 + 0.3 * i, 0.6 + 0.2 * i, 0.8 + 0.5 * i]
    return (ol.make_shared(ol.NICH, mu=p[0], kappa=p[1], sigmasq=p[2],
                           nu=p[3]), engine.nich_shared(*p))


def _column(rng, col, i, n):
    """-> (kind for _shared, dim, values)"""
    if col.startswith("dd"):
        dim = int(col[2:])
        p = rng.dirichlet(np.full(dim, 2.0))
        return "dd", dim, rng.choice(dim, n, p=p).astype(np.uint32)
    if col == "bb":
        return "bb", None, (rng.random(n) < 0.2 + 0.1 * (i % 6)).astype(
            np.uint32)
    if col == "gps":
        v = rng.poisson(3.0, n).clip(max=15).astype(np.uint32)
        v[_spread(rng, n, 3)] = 15
        return "gp", None, v
    if col == "gpbig":
        v = rng.poisson(3.0, n).astype(np.uint32)
        at = _spread(rng, n, 40)
        v[at] = rng.integers(300, 100001, at.size).astype(np.uint32)
        return "gp", None, v
    if col == "bnbs":
        v = rng.negative_binomial(2, 0.4, n).clip(max=7).astype(np.uint32)
        v[_spread(rng, n, 3)] = 7
        return "bnb", None, v
    assert col == "nich", col
    return "nich", None, rng.normal(0.7 * i - 1.0, 0.5 + 0.4 * i, n).astype(
        np.float32)


def make(name, n, k, seed=SEED):
    """-> (oracle shareds, engine shareds, values per feature, assign_packed)"""
    assign = (np.arange(n) % k).astype(np.uint32)
    osh, gsh, vals = [], [], []
    if name == "planted6":
        # workloads.planted's columns (four DirichletDiscrete(16), two reals
        # with structure) under hyper-parameters of their own
        vals = workloads.planted(n, seed=seed)[3]
        for i in range(6):
            o, g = _shared("dd", i, 16) if i < 4 else _shared("nich", i)
            osh.append(o)
            gsh.append(g)
        return osh, gsh, vals, assign
    rng = np.random.default_rng(seed)
    for i, col in enumerate(LISTS[name]):
        kind, dim, v = _column(rng, col, i, n)
        o, g = _shared(kind, i, dim)
        osh.append(o)
        gsh.append(g)
        vals.append(v)
    return osh, gsh, vals, assign


class Snapshot(object):
    """an oracle's state at one moment, with the accessors assert_same_state
    reads"""

    def __init__(self, orc):
        self.F = orc.F
        self.assign = orc.assign.copy()
        self._counts = orc.counts()
        self._groups = [[orc.get_group(f, g) for g in range(len(orc))]
                        for f in range(orc.F)]

    def __len__(self):
        return len(self._counts)

    def counts(self):
        return self._counts

    def get_group(self, f, g):
        return self._groups[f][g]


def set_low_entropy(orc, dataset_size):
    import ctypes
    orc.L.orc_mix_set_low_entropy.restype = None
    orc.L.orc_mix_set_low_entropy.argtypes = [ctypes.c_void_p, ctypes.c_int]
    orc.L.orc_mix_set_low_entropy(orc.h, dataset_size)


@functools.lru_cache(maxsize=None)
def oracle_sweeps(name, n, k, batch, seed, sweeps=2, alpha=1.0, d=0.2,
                  empty=1, dataset_size=None):
    """the oracle's state after each of `sweeps` sweeps in batches of `batch`
    rows (draws of sweep s from s * n on): computed once per argument list,
    shared by the tests, never changed"""
    osh, _, vals, assign = make(name, n, k)
    orc = ol.OracleMixture(alpha, d, osh)
    if dataset_size is not None:
        set_low_entropy(orc, dataset_size)
    orc.init_from_assignments(vals, assign, k, empty)
    st = ol.oracle().orc_rng_seed(seed)
    out = []
    for sweep in range(sweeps):
        for b in range(0, n, batch):
            orc.gibbs_batch(b, min(n, b + batch), st, sweep * n)
        out.append(Snapshot(orc))
    return tuple(out)
