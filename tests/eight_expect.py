"""Subjects of five to eight features for the held-out readers (predict,
predict_feature, sample_rows, their ensemble forms, coassign and the top-k
kernels), and the planted variants of the float64 law that tell whether a
test sees the features past the fourth.

TEST INFRASTRUCTURE (imported by tests only).

The eight-feature list is marginals_expect's (eight_rows, eight_shareds,
Member8, Ensemble8): DD5, BB, GP, NICH, DD70, BNB, DPD20 (beta0 = 0.1, two
query rows OTHER), DD3.  No second list is written here.

  eight         n = 2000, k = 40 + 3 empty, d = 0.5, alpha = 1: K = 43
  eight_swept   the same at alpha = 20 after two sweeps of 16-row batches:
                K = 79
  le_eight      LowEntropy, dataset_size = 3000, k = 40 + 1 empty, d = 0
  real_first    wide_rows.LISTS["real_first"] (NICH, DD8, GP, NICH, BB),
                n = 2000, k = 16 + 3 empty: a real feature first, a
                categorical one between reals
  eight3        Ensemble8 over SPECS_EIGHT3: K differs per member, the last
                member is wider than one staging tile of target 0, the
                middle one is swept

Like predict_expect's cases, query row 0 of the single-engine subjects
carries a DirichletDiscrete value no table row has (the widest DD's last).

`staged_geometry` restates the host's choice of (items, rows, tile) for the
staged predict_feature kernels: integer arithmetic on the subject's kinds,
the candidate count and K.

The planted variants (`planted_state`, `planted_mask`): what a float64 law
would be if a reader
  "drop"    left the last feature of index >= 4 out,
  "wrap"    took feature f's query words from feature f & 3 (f >= 4),
  "mask4"   read the observed mask through & 0xF.
"""
import copy

import numpy as np

import f64_scores as fx
import marginals_expect as mx
import oracle_lib as ol
import predict_expect as pe
import wide_rows
from test_f64_scores import build

OTHER = pe.OTHER
NQ = 100
SPECS_EIGHT3 = [dict(k=6, empty=2, alpha=1.0, d=0.0, sweeps=0),
                dict(k=19, empty=1, alpha=20.0, d=0.5, sweeps=1),
                dict(k=40, empty=3, alpha=5.0, d=0.25, sweeps=0)]
# the fixed masks of the issue: only features >= 4, only features < 4,
# alternating
FIXED_MASKS = (0xF0, 0x0F, 0xAA)
TARGETS8 = (0, 3, 4, 6, 7)

#            name: (list, k, empty, d, sweeps, LowEntropy dataset size)
SUBJECTS = {
    "eight": ("eight", 40, 3, 0.5, 0, None),
    "eight_swept": ("eight", 40, 3, 0.5, 2, None),
    "le_eight": ("eight", 40, 1, 0.0, 0, 3000),
    "real_first": ("real_first", 16, 3, 0.5, 0, None),
}
NAMES = list(SUBJECTS)


class Wide(pe.Case):
    """a predict_expect.Case over one of this module's lists"""

    def __init__(self, name):
        lst, k, empty, d, sweeps, le = SUBJECTS[name]
        self.name, self.config = name, lst
        self.n, self.k, self.empty, self.d = 2000, k, empty, d
        self.sweeps, self.le, self.nq, self.dim = sweeps, le, NQ, None
        self.unassigned = False
        self.assign0 = (np.arange(self.n) % k).astype(np.uint32)
        if lst == "eight":
            self.vals = mx.eight_rows(self.n, pe.workloads.SEED)
            self.osh, self.gsh = mx.eight_shareds(0)
            qvals = mx.eight_rows(self.nq, pe.QSEED)
        else:
            self.osh, self.gsh, self.vals, _ = wide_rows.make(lst, self.n, k)
            _, _, qvals, _ = wide_rows.make(lst, self.nq, k, seed=pe.QSEED)
        self.qvals = [q.copy() for q in qvals]
        dds = [f for f, sh in enumerate(self.osh) if sh.kind == ol.DD]
        f = max(dds, key=lambda i: self.osh[i].dim)
        # the widest DirichletDiscrete's last value has no row in the table,
        # and query row 0 carries it
        self.vals[f][self.vals[f] == self.osh[f].dim - 1] = 0
        self.qvals[f][0] = self.osh[f].dim - 1
        for f, sh in enumerate(self.osh):
            if sh.kind == ol.DPD:
                self.qvals[f][[1, 2]] = OTHER
        self.alpha = 20.0 if sweeps else 1.0
        self.orc, self.st = build(self.osh, self.vals, self.assign0, k,
                                  empty, self.alpha, d, sweeps, le)
        self.K = len(self.orc)
        self._expect = None
        self._f64 = None


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Wide(name)
    return _CASES[name]


_ENSEMBLES = {}


def eight3():
    """the ensemble of the module docstring, built once"""
    if "eight3" not in _ENSEMBLES:
        _ENSEMBLES["eight3"] = mx.Ensemble8(specs=SPECS_EIGHT3, n=600, nq=NQ)
    return _ENSEMBLES["eight3"]


def eight3_head(n):
    """eight3 with its first n held-out rows only (the members are shared)"""
    key = "eight3_%d" % n
    if key not in _ENSEMBLES:
        ens = copy.copy(eight3())
        ens.nq, ens.qvals = n, [v[:n] for v in ens.qvals]
        ens._expect, ens._f64 = {}, None
        _ENSEMBLES[key] = ens
    return _ENSEMBLES[key]


def repeat_rows(qvals, n):
    """the query columns cycled to n rows"""
    return [np.resize(v, n) for v in qvals]


def masks_for(n, F, seed):
    """feature_expect.random_masks with the fixed masks on three rows each
    (rows 3 .. 11), junk bits above F kept on every third row"""
    import feature_expect as fe
    m = fe.random_masks(n, F, seed)
    at = 3
    for fixed in FIXED_MASKS:
        for _ in range(3):
            if at < n:
                m[at] = (m[at] & np.uint32(0xFF000000)) | np.uint32(
                    fixed & ((1 << F) - 1))
            at += 1
    return m


# ---------------------------------------------------------------------------
# the staged predict_feature kernels' launch geometry, restated

BLOCK = 256                  # threads of a workgroup
FEATURE_ROWS_MAX = 32        # rows a workgroup may touch
FEATURE_LDS_BUDGET = 48 * 1024


def is_cat(kind):
    return kind in (ol.DD, ol.DPD)


def terms_after(kinds, target):
    """LDS planes of the features after the target: a categorical feature
    stages two words (numerator and denominator), every other kind one"""
    return sum(2 if is_cat(k) else 1 for k in kinds[target + 1:])


def feature_lds(terms, tile, rows):
    return (1 + terms) * (tile + 1) * rows * 4


def staged_geometry(kinds, target, C, K, n_rows):
    """-> dict(items, rows, tile, tiles, lds, planes) as the host's launch
    takes them for C candidates, K groups (an ensemble's largest) and
    n_rows query rows in the chunk"""
    S = C + 1
    items = BLOCK
    if (items - 1) // S + 2 > FEATURE_ROWS_MAX:
        items = (FEATURE_ROWS_MAX - 2) * S + 1
    rows = min((items - 1) // S + 2, n_rows + 1)
    terms = terms_after(kinds, target)
    per_k = feature_lds(terms, 0, rows)
    tile = max(min(K, FEATURE_LDS_BUDGET // per_k - 1), 1)
    return dict(items=items, rows=rows, tile=tile, tiles=-(-K // tile),
                lds=feature_lds(terms, tile, rows), planes=1 + terms)


# ---------------------------------------------------------------------------
# planted variants of the float64 law

VARIANTS = ("drop", "wrap", "mask4")


def planted_state(state, qcols, variant):
    """-> (state, query columns) of a reader that is wrong past the fourth
    feature in the way `variant` names (module docstring); "mask4" changes
    nothing here (see planted_mask)."""
    F = len(state.feats)
    if variant == "drop":
        assert F > 4
        s = copy.copy(state)
        s.feats, s.cols, s.stats = (state.feats[:-1], state.cols[:-1],
                                    state.stats[:-1])
        return s, list(qcols[:-1])
    if variant == "wrap":
        out = list(qcols)
        for f in range(4, F):
            src = np.asarray(qcols[f & 3])
            kind = state.feats[f].kind
            # the WORDS of feature f & 3 read as feature f's
            words = ol.value_words(state.feats[f & 3].kind, src)
            if kind == fx.NICH:
                out[f] = words.view(np.float32).copy()
            else:
                w = words.copy()
                if kind in (fx.DD, fx.BB):
                    # stays inside the table, as a plant must
                    dim = 2 if kind == fx.BB else state.feats[f].dim
                    w = w % np.uint32(dim)
                out[f] = w
        return state, out
    assert variant == "mask4", variant
    return state, list(qcols)


def planted_mask(observed, variant, drop=None):
    """the masks a reader with `variant` acts on; under masks "drop" leaves
    feature `drop` (>= 4) out by never observing it"""
    observed = np.asarray(observed, np.uint32)
    if variant == "mask4":
        return observed & np.uint32(0xF)
    if variant == "drop":
        assert drop >= 4
        return observed & ~np.uint32(1 << drop)
    return observed
