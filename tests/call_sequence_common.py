"""Inputs, step tables and references of the call-sequence tests (tests/test_call_sequences.py runs the tables on the GPU,
one fresh process per family through tests/call_sequence_worker.py; tests/test_call_sequence_host.py certifies them on the
CPU) and the structure-hint generator of tests/test_abi_entries_exact.py.

libfigh carries state from call to call: named workspace slots that unrelated entries share, the cached per-tile hint of
figh_tsqr_structured, the zero hint that remembers how much it zeroed, the poisoned buffers of the streamed merge tree, the
process-wide null-pivot threshold, the per-handle active rows.  Every other suite calls an entry as if it were the only call
of the process.  Here a family is ONE ordered table of steps: the worker performs them in order in a fresh process (every
slot starts empty, every cache cold) and stores the raw results; the parent rebuilds the same inputs from the same seeds
and applies to every step the metric its entry has in the existing suites.  A step that repeats an earlier call names it
in ``repeat_of``; ``bits`` lists the results that must then be equal bit for bit (only what figh.h documents as
reproducible or the suite already compares with a mirror).

Nothing here needs a device or the library.  The structured family takes its wrench and row-block cases from
test_qr_structured_graded (its generators and checks are that module's), the filters from preprocessing_common (SciPy).
"""
import functools
from collections import namedtuple

import numpy as np

import qr_graded_common as qg

TOL_QR = 1e-8
SENT = -7.25e77  # pre-fill of output buffers (finite, nothing computes it)

# tag: unique in the family; op: key of the worker's RUN and the parent's CHECK tables; args: the inputs (arrays and
# generator objects, shared by reference between a step and its repeats); repeat_of: tag of the step this one repeats;
# bits: result names that must equal that step's bit for bit
Step = namedtuple("Step", "tag op args repeat_of bits")


def _step(tag, op, args, repeat_of=None, bits=()):
    return Step(tag, op, args, repeat_of, tuple(bits))


# ------------------------------------------------------------------------------------------------ structure-hint inputs
def hint_list(rng, pattern, nfirst, rb, n, tau_first=False):
    """``nfirst`` first columns in [0, n] for row blocks of ``rb`` rows.  pattern: "zeros", "ascending", "descending",
    "random" (unsorted, one block at 0).  In sorted order the k-th value is at most k rb / 3, so that the t leading columns
    are supported on at least 3 t rows (the stack stays full rank and well conditioned: the forward metric applies).
    ``tau_first``: the block with the largest value gets first == n -- no column of W at all, only its tau."""
    if pattern == "zeros":
        raw = np.zeros(nfirst, dtype=np.int64)
    elif pattern in ("ascending", "descending"):
        raw = (np.arange(nfirst) * n) // nfirst
    else:
        assert pattern == "random", pattern
        raw = np.sort(rng.integers(0, n, nfirst))
        raw[0] = 0
    s = np.minimum(np.sort(raw), (np.arange(nfirst) * rb) // 3)
    s = np.minimum(s, max(n - 1, 0))
    if tau_first and nfirst > 1:
        s[-1] = n
    if pattern == "descending":
        s = s[::-1]
    elif pattern == "random":
        s = s[rng.permutation(nfirst)]
    return np.ascontiguousarray(s, dtype=np.int32)


class Hinted:
    """Graded integer matrix with the zero structure a host hint describes: ``len(first)`` row blocks of ``rb`` rows; in
    block b the gathered columns < first[b] are exactly zero and EVERY row of the block carries +-2^10 (the largest entry
    there is) at column first[b] -- a hint applied to the wrong rows or the wrong tile drops entries of the size of the
    column norm.  ``gather``: the n columns are an unsorted selection out of ld = n + 7; ``nweights`` > 0: that many
    power-of-two row-block weights; ``dense``: no zero anywhere (what a run WITHOUT a hint must still read in full)."""

    def __init__(self, rng, rb, first, n, profile, with_tau=False, gather=True, nweights=0, dense=False):
        first = np.asarray(first, dtype=np.int32)
        self.first, self.rb, self.n, self.nfirst = first, int(rb), int(n), len(first)
        self.rows = rows = self.rb * self.nfirst
        self.nc = n + (1 if with_tau else 0)
        self.ld = ld = n + 7 if gather else n
        lo, hi = qg.PROFILES[profile]
        Mw = qg.int_matrix(rng, rows, ld)
        self.idx = rng.permutation(ld)[:n].astype(np.int32) if gather else None
        idx = self.idx if gather else np.arange(n)
        sw = qg.graded_scales(rng, ld, lo, hi)
        sw[idx[qg.small_positions(n)]] = lo
        if dense:
            Mw[Mw == 0] = 1.0
        else:
            f_row = np.repeat(first.astype(np.int64), self.rb)
            Gm = Mw[:, idx]
            Gm[np.arange(n)[None, :] < f_row[:, None]] = 0.0
            r = np.flatnonzero(f_row < n)
            Gm[r, f_row[r]] = qg.INT_MAX * rng.choice([-1.0, 1.0], len(r))
            Mw[:, idx] = Gm
        self.Mw, self.sw, self.cols = Mw, sw, idx
        self.mt = self.st = None
        if with_tau:
            mt = qg.int_matrix(rng, rows, 1)[:, 0]
            mt[mt == 0] = 1.0  # (a block with first == n lives on its tau alone)
            self.mt, self.st = mt, int(rng.integers(lo, hi + 1))
        self.wexp = rng.integers(-1, 2, nweights) if nweights else None
        if nweights:
            assert rows % nweights == 0

    def A(self):
        """The ld-wide matrix as the device gets it (float64, exact)."""
        return self.Mw * np.ldexp(1.0, self.sw)

    def tau(self):
        return None if self.mt is None else self.mt * 2.0 ** self.st

    def weights(self):
        return None if self.wexp is None else np.ldexp(1.0, self.wexp)

    def M(self):
        """Integer columns of [W[:, idx] tau]."""
        Mg = self.Mw[:, self.cols]
        return Mg if self.mt is None else np.c_[Mg, self.mt]

    def s(self):
        sg = self.sw[self.cols]
        return sg if self.mt is None else np.r_[sg, self.st]

    def gram(self):
        row_exp = None if self.wexp is None else np.repeat(self.wexp, self.rows // len(self.wexp))
        return qg.exact_gram(self.M(), self.s(), row_exp)

    def gathered(self):
        """[W[:, idx] tau] with the row weights applied, float64 (exact): what a host QR factors."""
        X = self.M() * np.ldexp(1.0, self.s())
        if self.wexp is not None:
            X = X * np.repeat(np.ldexp(1.0, self.wexp), self.rows // len(self.wexp))[:, None]
        return X

    def forward(self):
        return self.rows >= 2 * self.nc


# (id, n, tau, rows per block, nfirst, pattern, a block with first == n, gathered from a wider ld, row-block weights, profile).
# nc = n + tau in {1, 16, 17, 64, 65, 80, 81}: one wave, the two instantiations of tsqr2_kernel (split at 64 | 65, each with
# and without tau) and 81, where the hint is ignored; rows per block in {1, 37, 64, 100, 640}: tiles that straddle blocks,
# many blocks per tile; fewer than 64 rows in all; nfirst in {1, 6, 7, 640}; eight weights: nblocks != nfirst
STRUCTURED_CASES = [
    ("n1_1x37_ragged", 1, False, 37, 1, "zeros", False, False, 0, "wide"),
    ("n1tau_640x1", 1, True, 1, 640, "random", True, True, 8, "wide"),
    ("n16_6x100_ascending", 16, False, 100, 6, "ascending", False, True, 0, "wide"),
    ("n16_7x1_seven_rows", 16, False, 1, 7, "random", False, True, 0, "tiago"),
    ("n17_7x37_descending", 17, False, 37, 7, "descending", False, True, 0, "tiago"),
    ("n16tau_6x640_random_weights", 16, True, 640, 6, "random", True, True, 8, "wide"),
    ("n64_6x64_random_weights", 64, False, 64, 6, "random", False, True, 8, "wide"),
    ("n64_7x640_ascending", 64, False, 640, 7, "ascending", False, False, 0, "tiago"),
    ("n64_640x1_descending", 64, False, 1, 640, "descending", False, True, 0, "wide"),
    ("n63tau_6x100_zeros", 63, True, 100, 6, "zeros", False, True, 0, "wide"),
    ("n64tau_6x100_descending_taufirst", 64, True, 100, 6, "descending", True, True, 0, "wide"),
    ("n65_6x37_ascending", 65, False, 37, 6, "ascending", False, True, 0, "tiago"),
    ("n79tau_6x100_ascending", 79, True, 100, 6, "ascending", False, True, 0, "wide"),
    ("n79tau_640x1_random_weights", 79, True, 1, 640, "random", False, True, 8, "wide"),
    ("n79tau_7x64_random_taufirst_weights", 79, True, 64, 7, "random", True, True, 8, "tiago"),
    ("n80_7x100_descending", 80, False, 100, 7, "descending", False, True, 0, "wide"),
    ("n79tau_1x37_ragged", 79, True, 37, 1, "zeros", False, True, 0, "wide"),
    ("n81_6x100_descending_hint_ignored", 81, False, 100, 6, "descending", False, True, 0, "wide"),
    ("n80tau_7x64_random_hint_ignored", 80, True, 64, 7, "random", True, True, 8, "tiago"),
]


def structured_case(case):
    """The Hinted input of a STRUCTURED_CASES entry (seeded by its position-independent fields)."""
    name, n, tau, rb, nfirst, pattern, tau_first, gather, nweights, profile = case
    rng = np.random.default_rng([n, int(tau), rb, nfirst, len(pattern), int(tau_first), nweights])
    first = hint_list(rng, pattern, nfirst, rb, n, tau_first=tau_first and tau)
    return Hinted(rng, rb, first, n, profile, with_tau=tau, gather=gather, nweights=nweights)


class Selected:
    """Input of figh_tsqr_selected with nblocks > 0: ``nblocks`` row blocks of ``rb`` rows in the reference layout (14
    columns per link, one link per block), row block b exactly zero in the reference columns < 14 b, a fifth of the
    columns dead (all zero: the elimination drops them); graded, with tau."""

    def __init__(self, rng, rb, nblocks, profile):
        lo, hi = qg.PROFILES[profile]
        self.rb, self.nblocks, self.rows, self.ncols = rb, nblocks, rb * nblocks, 14 * nblocks
        dead = np.sort(rng.choice(self.ncols, self.ncols // 5, replace=False))
        self.kept = np.setdiff1d(np.arange(self.ncols), dead)
        self.n = len(self.kept)
        M = qg.int_matrix(rng, self.rows, self.ncols)
        M[:, dead] = 0.0
        blk = np.repeat(np.arange(nblocks), rb)
        M[np.arange(self.ncols)[None, :] < 14 * blk[:, None]] = 0.0
        self.M, self.s = M, qg.graded_scales(rng, self.ncols, lo, hi)
        self.mt, self.st = qg.int_matrix(rng, self.rows, 1)[:, 0], int(rng.integers(lo, hi + 1))

    def A(self):
        return self.M * np.ldexp(1.0, self.s)

    def tau(self):
        return self.mt * 2.0 ** self.st

    def colsq(self):
        return np.diag(qg.exact_gram(self.M, self.s)).copy()

    def tol_e(self):
        cs = self.colsq()
        return 0.5 * cs[cs > 0].min()

    def gram(self):
        return qg.exact_gram(np.c_[self.M[:, self.kept], self.mt], np.r_[self.s[self.kept], self.st])


class Deficient:
    """Graded integer matrix with exact dependencies (every third column, qg.make_dependent): the input of the null-pivot
    rule's column bound (test_qr_graded.test_null_pivot_rule_graded_column_bound)."""

    def __init__(self, rng, rows, n, profile):
        lo, hi = qg.PROFILES[profile]
        self.rows, self.n = rows, n
        M = qg.int_matrix(rng, rows, n)
        s = qg.graded_scales(rng, n, lo, hi, qg.small_positions(n))
        self.dep, self.base = qg.make_dependent(rng, M, s, n, lo)
        self.M, self.s = M, s

    def A(self):
        return self.M * np.ldexp(1.0, self.s)

    def gram(self):
        return qg.exact_gram(self.M, self.s)

    def min_base_pivot(self):
        G = self.gram()
        return float(np.diag(qg.cholesky_ld(G[np.ix_(self.base, self.base)])).min())


class Stack:
    """A stack of graded integer triangles (qg.graded_triangles); ``n_free`` is not None: with exact dependencies among
    its first n_free columns (the input of figh_tsqr_merge_base)."""

    def __init__(self, seed, nc, count, profile, n_free=None):
        rng = np.random.default_rng(seed)
        self.nc, self.count, self.n_free = nc, count, n_free
        self.T, self.s = qg.graded_triangles(rng, count, nc, profile)
        self.dep, self.base = [], list(range(nc))
        if n_free is not None:
            self.dep, self.base = qg.make_dependent(rng, self.T, self.s, n_free, qg.PROFILES[profile][0])

    def A(self):
        """count nc x nc float64 rows, stacked."""
        return (self.T * np.ldexp(1.0, self.s)).reshape(-1, self.nc)

    def gram(self):
        return qg.exact_gram(self.T.reshape(-1, self.nc), self.s)

    def base_free(self):
        return [k for k in self.base if k < self.n_free]


# --------------------------------------------------------------------------------------------------------- the families
def _hints():
    rng = np.random.default_rng([20, 1])
    n, rb, nf = 19, 100, 6  # 19 columns + tau = 20
    asc = hint_list(rng, "ascending", nf, rb, n)
    desc = hint_list(rng, "descending", nf, rb, n)
    D1 = Hinted(rng, 640, [0], n, "wide", with_tau=True, dense=True)
    S1 = Hinted(rng, rb, asc, n, "wide", with_tau=True)
    S2 = Hinted(rng, rb, desc, n, "wide", with_tau=True)
    D6 = Hinted(rng, 600, [0], n, "wide", with_tau=True, dense=True)
    S3 = Hinted(rng, 5000, hint_list(rng, "ascending", nf, 5000, n), n, "tiago", with_tau=True)
    D9 = Hinted(rng, 192000, [0], n, "tiago", with_tau=True, dense=True, gather=False)
    SEL = Selected(rng, rb, nf, "wide")
    S13 = Hinted(rng, rb, hint_list(rng, "descending", nf, rb, 79, tau_first=True), 79, "wide", with_tau=True)

    def t(tag, h, hint, rep=None):
        return _step(tag, "tsqr", dict(h=h, hint=hint), rep)

    return [t("01_dense_640", D1, False), t("02_S1", S1, True), t("03_S2_descending", S2, True),
            t("04_S1_again", S1, True, "02_S1"), t("05_S1_cache_hit", S1, True, "02_S1"),
            t("06_dense_600_no_zeros", D6, False), t("07_S3_slot_grows", S3, True), t("08_S1", S1, True, "02_S1"),
            t("09_dense_192000_zero_hint_grows", D9, False), t("10_dense_640", D1, False, "01_dense_640"),
            _step("11_selected_6_blocks", "tsqr_selected", dict(g=SEL)), t("12_S1", S1, True, "02_S1"),
            t("13_S_79_tau_other_instantiation", S13, True), t("14_S1", S1, True, "02_S1")]


def _merges():
    st = {}

    def S(nc, count, n_free=None):
        key = (nc, count, n_free)
        if key not in st:
            st[key] = Stack([nc, count, 0 if n_free is None else n_free, 4], nc, count, "wide", n_free)
        return st[key]

    def m(tag, nc, count, rep=None):
        return _step(tag, "merge", dict(g=S(nc, count)), rep)

    def mb(tag, nc, count):
        return _step(tag, "merge_base", dict(g=S(nc, count, nc - 1)))  # (with tau: the last column is free of the decision)

    return [m("01_50x17", 50, 17), m("02_50x300", 50, 300), m("03_50x17", 50, 17, "01_50x17"), m("04_33x17", 33, 17),
            m("05_64x16", 64, 16), mb("06_base_50x17", 50, 17), m("07_50x17", 50, 17, "01_50x17"), m("08_70x9", 70, 9),
            mb("09_base_70x33", 70, 33), m("10_70x9", 70, 9, "08_70x9"), m("11_20x4500_level_tree", 20, 4500),
            m("12_50x17", 50, 17, "01_50x17"), m("13_81x2_pair", 81, 2), m("14_64x16", 64, 16, "05_64x16")]


def _filter_case(d, L, cols, nblocks, q, seed):
    import preprocessing_common as pc
    form, b, a, zi, padlen = pc.design(*d)
    return dict(form=form, b=b, a=a, zi=zi, padlen=padlen, q=q, nblocks=nblocks, x=pc.make_signal(L, cols, nblocks, seed))


def _wide_filter():
    rng = np.random.default_rng([20, 3])
    T1 = Hinted(rng, 4000, [0], 96, "wide", gather=False, dense=True)
    T2 = Hinted(rng, 20011, [0], 193, "tiago", gather=False, dense=True)
    F1 = _filter_case(("sos", 4, None), 1003, 65, 3, 10, 5)  # work array 1057 x 195 doubles: larger than T1's packed blocks
    F2 = _filter_case(("tf", 5, None), 203, 5, 13, 3, 6)
    return [_step("01_tsqr_4000x96", "tsqr", dict(h=T1, hint=False)), _step("02_filtfilt_large", "filtfilt", F1),
            _step("03_tsqr_4000x96", "tsqr", dict(h=T1, hint=False), "01_tsqr_4000x96"),
            _step("04_filtfilt_small", "filtfilt", F2), _step("05_tsqr_20011x193", "tsqr", dict(h=T2, hint=False)),
            _step("06_filtfilt_large", "filtfilt", F1, "02_filtfilt_large", bits=("y",))]


UR10_FUSED_N = 4096


def _structured():
    import regressor_exact as rx
    from test_qr_structured_graded import BLOCK_CASES, WRENCH_CASES
    name, Nb, nlinks, n, dead, extra, with_tau, profile = {c[0]: c for c in WRENCH_CASES}["nc82"]
    assert 3 * Nb >= 16 * (n + with_tau)  # the force / torque split engages
    gw = qg.Wrench(np.random.default_rng([Nb, n, 0, len(profile)]), Nb, nlinks, n, *qg.PROFILES[profile], dead_links=dead,
                   extra_slots=extra, deps=False)
    wr = dict(g=gw, layout="force-link-compact", with_tau=with_tau)
    bname, spec, rows_b, btau = {c[0]: c for c in BLOCK_CASES}["wide"]  # grouped, mid and WIDE blocks (ncj 81, 200) and narrow ones
    gb = qg.RowBlocks(np.random.default_rng([rows_b, 4, 3, len(bname)]), rows_b, spec["nblocks"], spec["groups"],
                      *qg.PROFILES["wide"], inactive=spec["inactive"], deps=False, noise=spec["noise"],
                      k_block=spec["k_block"])
    bl = dict(g=gb, compact=True, with_tau=btau, want_tri=False)
    bl_tri = dict(g=gb, compact=True, with_tau=btau, want_tri=True)
    (q, v, a), _ = rx.reference("ur10", "unit", UR10_FUSED_N, rx.base_param(), seed=4)
    fused = dict(q=q, v=v, a=a, tau=np.random.default_rng(8).standard_normal(6 * UR10_FUSED_N))
    P = Hinted(np.random.default_rng([20, 4]), 2000, [0], 50, "wide", with_tau=True, dense=True)
    return [_step("01_wrench", "wrench", wr), _step("02_blocks", "blocks", bl), _step("03_fused_ur10", "fused", fused),
            _step("04_tsqr_workspace_triangles", "tsqr", dict(h=P, hint=False)), _step("05_wrench", "wrench", wr, "01_wrench"),
            _step("06_blocks", "blocks", bl, "02_blocks"), _step("07_blocks_block_tri", "blocks", bl_tri),
            _step("08_wrench", "wrench", wr, "01_wrench")]


STREAM_N = 209 + 64
BATCH_B = 3


def stream_total(model):
    """Samples on the device: the human model holds the BATCH_B trajectories of the batched step back to back (the first
    one is what its other steps read)."""
    return STREAM_N * (BATCH_B if model == "human" else 1)


@functools.lru_cache(maxsize=None)
def stream_inputs(model):
    """(param, (q, v, a), tau) of the streamed family for "tiago" (joint torques, all flags) or "human" (external wrench):
    stream_total samples from regressor_exact.reference, tau for the first STREAM_N of them."""
    import regressor_exact as rx
    param = rx.base_param(friction=True, inertia=True, offset=True) if model == "tiago" else rx.base_param(wrench=True)
    (q, v, a), _ = rx.reference(model, "unit", stream_total(model), param, seed=6)
    rps = int(rx.shipped_flat(model)["nv"]) if model == "tiago" else 6
    tau = np.random.default_rng([7, len(model)]).standard_normal(rps * STREAM_N)
    return param, (q, v, a), tau


@functools.lru_cache(maxsize=None)
def stream_kept(model):
    """The columns the streamed steps factor: those with an entry in the long-double reference W (TIAGo 245 of 336, the
    human model the 190 columns of its 19 links with a body: more than 80 either way)."""
    import regressor_exact as rx
    param, _, _ = stream_inputs(model)
    _, ref = rx.reference(model, "unit", stream_total(model), param, seed=6)
    return np.flatnonzero(np.any(ref.W != 0, axis=0)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def fused_kept():
    """UR10's kept columns (the golden elimination): the column list of the fused launch."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfg2_ur10.npz"))
    gone = set(int(x) for x in g["idx_e"])
    return np.array([c for c in range(84) if c not in gone], dtype=np.int32)


def _streamed():
    def s(tag, op, model, rep=None, bits=(), **kw):
        return _step(tag, op, dict(model=model, **kw), rep, bits)

    return [s("00_W_tiago", "rbuild", "tiago"), s("00_W_human", "rbuild", "human"),
            s("01_colsq_c64_tiago", "rcolsq", "tiago", chunk=64), s("01_colsq_c64_human", "rcolsq", "human", chunk=64),
            s("02_tsqr_c64_tau_tiago", "rtsqr", "tiago", chunk=64, norms=False),
            s("03_colsq_c64_tiago", "rcolsq", "tiago", "01_colsq_c64_tiago", chunk=64),
            s("03_colsq_c64_human", "rcolsq", "human", "01_colsq_c64_human", chunk=64),
            s("04_tsqr_norms_c150_tiago", "rtsqr", "tiago", chunk=150, norms=True),
            s("04_tsqr_norms_c150_human", "rtsqr", "human", chunk=150, norms=True),
            s("05_batch_human", "rbatch", "human"),
            s("06_tsqr_c64_tau_tiago", "rtsqr", "tiago", "02_tsqr_c64_tau_tiago", chunk=64, norms=False),
            s("07_gram_c0_tiago", "rgram", "tiago", chunk=0), s("07_gram_c0_human", "rgram", "human", chunk=0),
            s("08_colsq_c64_tiago", "rcolsq", "tiago", "01_colsq_c64_tiago", chunk=64),
            s("08_colsq_c64_human", "rcolsq", "human", "01_colsq_c64_human", chunk=64)]


def _settings():
    import regressor_exact as rx
    D = Deficient(np.random.default_rng([50, 4096, 4, 13]), 4096, 50, "wide")
    param = rx.base_param(friction=True, inertia=True, offset=True)
    (q, v, a), _ = rx.reference("ur10", "unit", 209, param, seed=2)
    prof = dict(model="ur10", param=param, q=q, v=v, a=a)
    (qt, vt, at), _ = rx.reference("tiago", "unit", 65, param, seed=2)
    ab = dict(model="tiago", param=param, q=qt, v=vt, a=at, rows_a=[0, 3, 7])
    return [_step("01_rule_off", "tsqr_deps", dict(g=D, rule=False)), _step("02_rule_on", "tsqr_deps", dict(g=D, rule=True)),
            _step("03_rule_off", "tsqr_deps", dict(g=D, rule=False), "01_rule_off"),
            _step("04_build_profile_0", "build_profile", dict(prof, level=0)),
            _step("05_build_profile_1", "build_profile", dict(prof, level=1), "04_build_profile_0", bits=("W",)),
            _step("06_build_profile_2", "build_profile", dict(prof, level=2), "04_build_profile_0", bits=("W",)),
            _step("07_handle_B_between_A_settings", "active_rows_ab", ab)]


_FAMILIES = {"hints": _hints, "merges": _merges, "wide_filter": _wide_filter, "structured": _structured,
             "streamed": _streamed, "settings": _settings}
FAMILIES = tuple(_FAMILIES)

# what each family pins (DESIGN.md repeats it)
STATE = {
    "hints": "tile_hint's cache (pointer, rows, list), kWsTileHint / kWsHintFirst growth, zero_tile_hint's zeroed length, "
             "kWsSelectedHint",
    "merges": "the poisoned stream buffers of both instantiations across nc and count, kWsMergeA/B, kWsOneTri, kWsReveal*",
    "wide_filter": "kWsWideBlkOrFilter between the blocked TSQR and figh_filtfilt_cols",
    "structured": "kWsForceOrBlockTri/R, kWsLevel0TriOrWrench, kWsForceCols, kWsBlockStack, kWsBlocks*Tri",
    "streamed": "kWsChunkW, kWsChunkNormsOrCols (doubles, int32, doubles), kWsChunkStack, kWsChunkTau, kWsLinkPos, kWsBatchPair",
    "settings": "figh_tsqr_null_pivot_tol, figh_profile_enable, figh_model_set_active_rows per handle",
}
# results that are documented as reproducible (figh.h) or already compared bit for bit with a mirror
BIT_EXACT_RESULTS = ("W", "colsq_chain", "colsq_fused", "apply", "y")


@functools.lru_cache(maxsize=None)
def steps(family):
    """The step table of a family: the worker's call list and the parent's reference list."""
    table = _FAMILIES[family]()
    tags = [s.tag for s in table]
    assert len(set(tags)) == len(tags), "duplicate step tags in %s" % family
    for s in table:
        assert s.repeat_of is None or tags.index(s.repeat_of) < tags.index(s.tag), "%s repeats a later step" % s.tag
        assert set(s.bits) <= set(BIT_EXACT_RESULTS), "%s asserts bits of a result that is not documented as reproducible" % s.tag
    return table


def result_key(tag, name):
    return "%s/%s" % (tag, name)


# -------------------------------------------------------------------------------------- what the references can certify
def certify(step):
    """The preconditions of the step's metric, as a dict of booleans and figures: ``guard`` (cond^2 2^-64 <= 0.1 cond u
    wherever the forward metric runs), ``tall`` (rows >= 2 nc for a full-rank step that runs it), ``pivot`` (the smallest
    true pivot of a step with exact dependencies, to be >= 3 tol_qr).  Ops whose reference is a kernel-built W read back
    (long-double Gram, backward metric only) or a bit-exact mirror certify nothing here."""
    U = 2.0 ** -53

    def guard(G):
        cond = qg.equilibrated_cond(qg.cholesky_ld(G))
        return dict(cond=cond, guard=cond * cond * 2.0 ** -64 <= 0.1 * cond * U)

    op, a = step.op, step.args
    if op == "tsqr":
        h = a["h"]
        return dict(guard(h.gram()), tall=h.rows >= 2 * h.nc) if h.forward() else dict(tall=None)
    if op == "tsqr_selected":
        g = a["g"]
        return dict(guard(g.gram()), tall=g.rows >= 2 * (g.n + 1))
    if op == "merge":
        g = a["g"]
        return dict(guard(g.gram()), tall=g.count * g.nc >= 2 * g.nc or g.count == 1)
    if op == "merge_base":
        g = a["g"]
        b = g.base_free()
        G = g.gram()[np.ix_(b, b)]
        return dict(guard(G), pivot=float(np.diag(qg.cholesky_ld(G)).min()))
    if op == "tsqr_deps":
        return dict(pivot=a["g"].min_base_pivot())
    if op == "wrench":
        g = a["g"]
        return dict(guard(g.gram(a["with_tau"])), tall=g.rows >= 2 * (g.n + 1))
    if op == "blocks":
        g = a["g"]
        return dict(guard(np.asarray(g.gram(a["with_tau"]), dtype=np.float64)), tall=True)
    return {}
