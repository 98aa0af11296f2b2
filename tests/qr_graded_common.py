"""Exact references for the column-wise QR accuracy tests (tests/test_qr_graded.py, the helper tests in test_host_logic.py).

Inputs are integer matrices with entries of a few bits, graded by power-of-two column scales: their fp64 Gram matrix is
exact whatever the summation order (every partial sum is an integer below 2^53), and scaling it by 2^(s_i + s_j) gives
the exact Gram of the graded matrix.  The reference R is the Cholesky factor of that Gram in extended precision; its
error is invariant under column scaling, so it is accurate column by column (about cond^2 * 1e-19, cond of the
column-equilibrated matrix), which is what the metrics below need: every metric is divided by the norms of the columns it
reads, never by the largest entry of the problem.
"""
import numpy as np

INT_MAX = 2 ** 10
# column-wise backward tolerance of the TSQR kernels (test_qr_graded.py; the normal-equation terms and the per-row-block
# residuals of test_reductions_graded.py, formed from R, share it): measured 5.2e-15 on an MI355X (rfactor 20011 x 511,
# wide profile; 7.7e-15 with dependent columns)
TOL_BACKWARD = 1e-13
# power-of-two column-scale ranges (lo, hi) of the graded inputs: TIAGo's kept columns span 7e4 in norm; "wide" is 2^60
PROFILES = {"tiago": (-10, 7), "wide": (-30, 30)}


def int_matrix(rng, rows, n, lo=-INT_MAX, hi=INT_MAX):
    """Integer entries in [lo, hi], stored as float64."""
    return rng.integers(lo, hi + 1, (rows, n)).astype(np.float64)


def graded_scales(rng, n, lo, hi, small=()):
    """Power-of-two exponents in [lo, hi], unsorted; the columns in ``small`` get ``lo`` (the smallest scale)."""
    s = rng.integers(lo, hi + 1, n)
    for j in small:
        if 0 <= j < n:
            s[j] = lo
    return s


def small_positions(n, edges=(16, 64, 80, 192, 256, 320, 336, 384, 400)):
    """First, last and the columns on both sides of the panel / chunk boundaries of the TSQR kernels."""
    pos = {0, n - 1}
    for e in edges:
        pos.update((e - 1, e))
    return sorted(p for p in pos if 0 <= p < n)


def graded_triangles(rng, count, nc, profile):
    """count integer upper triangles, diagonally weighted (|diag| in [512, 1024], small off-diagonal entries) so that the
    stack stays well conditioned after equilibration, graded by power-of-two column scales."""
    B = max(1, 1024 // (4 * int(np.ceil(np.sqrt(nc)))))
    T = rng.integers(-B, B + 1, (count, nc, nc)).astype(np.float64)
    i = np.arange(nc)
    T[:, i, i] = rng.integers(512, 1025, (count, nc)) * rng.choice([-1.0, 1.0], (count, nc))
    T = np.triu(T)
    lo, hi = PROFILES[profile]
    return T, graded_scales(rng, nc, lo, hi, small_positions(nc) + [nc // 2])


def exact_gram(M, s=None, row_exp=None):
    """Exact Gram matrix of ``M * 2^s`` (columns) with rows scaled by ``2^row_exp`` (per row, or None).

    ``M`` must hold integers.  Every product and partial sum of the per-exponent integer Gram is an integer of at most 53
    bits, so BLAS computes it exactly in any order; the power-of-two scalings and the sum over the (few) row exponents
    are exact as long as the combined integers stay within 53 bits, which is asserted."""
    M = np.asarray(M, dtype=np.float64)
    assert np.array_equal(M, np.round(M)), "exact_gram needs integer entries"
    n = M.shape[1]
    s = np.zeros(n, dtype=np.int64) if s is None else np.asarray(s, dtype=np.int64)
    if row_exp is None:
        row_exp = np.zeros(M.shape[0], dtype=np.int64)
    row_exp = np.asarray(row_exp, dtype=np.int64)
    exps = np.unique(row_exp)
    amax = float(np.abs(M).max(initial=0.0))
    # the sum over row exponents e of 4^(e - e_min) * (integer Gram of those rows): one integer below 2^53
    span = 4.0 ** float(exps.max() - exps.min()) if exps.size else 1.0
    assert M.shape[0] * amax * amax * span < 2.0 ** 53, "Gram not exact in float64"
    G = np.zeros((n, n))
    for e in exps:
        Me = M[row_exp == e]
        G += (Me.T @ Me) * 4.0 ** float(e - exps.min())
    G *= 4.0 ** float(exps.min()) if exps.size else 1.0
    return G * np.ldexp(1.0, (s[:, None] + s[None, :]).astype(np.int64))


def check_longdouble():
    assert np.finfo(np.longdouble).nmant >= 63, "the exact references need an 80-bit (or wider) long double"


def cholesky_ld(G):
    """Upper-triangular R with R^T R = G, in np.longdouble (right-looking, vectorised over the trailing block)."""
    check_longdouble()
    A = np.array(G, dtype=np.longdouble)
    n = A.shape[0]
    R = np.zeros_like(A)
    for k in range(n):
        d = A[k, k]
        if not d > 0:
            raise np.linalg.LinAlgError("Gram matrix not positive definite at column %d" % k)
        r = np.sqrt(d)
        R[k, k] = r
        row = A[k, k + 1:] / r
        R[k, k + 1:] = row
        A[k + 1:, k + 1:] -= np.outer(row, row)
    return R


def positive_diag(R):
    """R with its rows' signs flipped so that diag(R) >= 0 (the factor is unique up to these signs)."""
    R = np.array(R)
    sg = np.where(np.diag(R) < 0, -1.0, 1.0)
    return R * sg[:, None].astype(R.dtype)


def col_norms(G):
    return np.sqrt(np.diag(np.asarray(G, dtype=np.float64)))


def backward_err(R, G):
    """max_ij |R^T R - G|_ij / (|a_i| |a_j|), R^T R formed in long double (its own rounding is then ~n * 1e-19)."""
    Rl = np.asarray(R, dtype=np.longdouble)
    nrm = np.asarray(col_norms(G), dtype=np.longdouble)
    nrm = np.where(nrm > 0, nrm, 1)
    E = np.abs(Rl.T @ Rl - np.asarray(G, dtype=np.longdouble)) / np.outer(nrm, nrm)
    return float(E.max(initial=0.0))


def forward_err(R, R_ref, G):
    """max_j |R[:, j] - R_ref[:, j]| / |a_j| after both diagonals are made positive."""
    D = np.asarray(positive_diag(R), dtype=np.longdouble) - positive_diag(np.asarray(R_ref, dtype=np.longdouble))
    nrm = np.asarray(col_norms(G), dtype=np.longdouble)
    nrm = np.where(nrm > 0, nrm, 1)
    return float((np.sqrt((D * D).sum(axis=0)) / nrm).max(initial=0.0))


def diag_err(R, R_ref, G):
    """max_k | |R_kk| - |R_ref_kk| | / |a_k|: the quantity the base-parameter decision reads."""
    d = np.abs(np.diag(np.asarray(R, dtype=np.longdouble))) - np.abs(np.diag(np.asarray(R_ref, dtype=np.longdouble)))
    nrm = np.asarray(col_norms(G), dtype=np.longdouble)
    nrm = np.where(nrm > 0, nrm, 1)
    return float((np.abs(d) / nrm).max(initial=0.0))


def equilibrated_cond(R_ref):
    """Condition number of the column-equilibrated matrix, from the reference factor."""
    R = np.asarray(R_ref, dtype=np.float64)
    nrm = np.sqrt((R * R).sum(axis=0))
    return float(np.linalg.cond(R / np.where(nrm > 0, nrm, 1)))


def normwise_backward_err(R, G):
    """The suite's older, norm-wise check: max |R^T R - G| / max |G|."""
    return float(np.abs(R.T @ R - G).max() / np.abs(G).max())


# ------------------------------------------------------------------------------------ the null-pivot rule's column bound
TOL_QR = 1e-8          # qrdecomposition.py:205-221: |R_kk| > tol_qr decides the base columns
NULL_TOL = TOL_QR / 64  # the rule's threshold per level-0 triangle (_lib.null_pivots)


def null_bound(G, rows, pieces):
    """(Shared by test_qr_structured_graded.py and test_streamed_columnwise.py.)  Column-wise bound with the null-pivot rule
    on: TOL_BACKWARD + (tol_qr / 64) sqrt(T) (|a_i| + |a_j|) / (|a_i| |a_j|), T from _host.null_rule_triangles."""
    from figaroh_plus_amd._host import null_rule_triangles
    nrm = col_norms(G)
    nrm = np.where(nrm > 0, nrm, 1.0)
    T = null_rule_triangles(rows, pieces)
    return TOL_BACKWARD + NULL_TOL * np.sqrt(T) * (nrm[:, None] + nrm[None, :]) / np.outer(nrm, nrm), nrm


def null_rule_check(R, G, rows, pieces, base, n, tag, record_property, rule):
    assert np.flatnonzero(np.abs(np.diag(R))[:n] > TOL_QR).tolist() == base, "%s: base set differs" % tag
    bound, nrm = null_bound(G, rows, pieces)
    if not rule:
        bound = np.full_like(bound, TOL_BACKWARD)
    Rl = np.asarray(np.triu(R), dtype=np.longdouble)
    E = np.abs(Rl.T @ Rl - np.asarray(G, dtype=np.longdouble)) / np.outer(nrm, nrm).astype(np.longdouble)
    record_property("%s:backward_over_bound" % tag, "%.3e" % float((E / bound).max()))
    assert (E <= bound).all(), "%s: column-wise backward error above the bound" % tag


# ------------------------------------------------------------------------------------ structured generators (wrench, blocks)
def make_dependent(rng, X, s, n, lo, same_class=None):
    """(Shared by test_qr_graded.py and the structured tests.)  Make every third column k < n (k % 3 == 2) of ``X`` (last axis = columns) an exact combination, with coefficients
    +-1 .. +-3, of up to three earlier base columns of scale <= 2^-8 within 2^4 of each other; ``s`` is updated in place.
    ``same_class`` (one label per column, optional): the sources of a dependent column carry its label, so that a zero
    pattern shared by the columns of a class survives.  Returns (dependent, base) column lists."""
    dep = [k for k in range(2, n) if k % 3 == 2]
    base = [k for k in range(X.shape[-1]) if k not in dep]
    cls = np.zeros(X.shape[-1], dtype=np.int64) if same_class is None else np.asarray(same_class)
    for k in list(dep):
        cand = [i for i in base if i < k and cls[i] == cls[k] and s[i] <= -8]
        if not cand:
            same = [i for i in base if i < k and cls[i] == cls[k]]
            if not same:  # nothing of its class in front of it: the column stays a base column
                dep.remove(k)
                base.append(k)
                continue
            s[same[0]] = max(lo, -8)
            cand = [same[0]]
        anchor = s[rng.choice(cand)]
        src = [i for i in cand if anchor <= s[i] <= anchor + 4]
        src = list(rng.choice(src, min(3, len(src)), replace=False))
        c = rng.integers(1, 4, len(src)) * rng.choice([-1, 1], len(src))
        X[..., k] = sum(int(ci) * X[..., i] * 2.0 ** int(s[i] - anchor) for ci, i in zip(c, src))
        s[k] = anchor
    return dep, sorted(base)


def device_column(c, link_stride=14, link_pos=None):
    """Device column of reference column ``c`` (14 per link) as figh_select_columns numbers it: the reference layout
    (stride 14), link-padded (16 l + s) or link-compact (16 pos[l] + s)."""
    c = np.asarray(c, dtype=np.int64)
    link = c // 14 if link_pos is None else np.maximum(np.asarray(link_pos)[c // 14], 0)
    return link * link_stride + c % 14


def force_column(dev_col):
    """Column of the force region of the force-compact layout that holds device column 16 p + s (s >= 6) of the torque
    rows (split_force_columns_kernel): 16 (p >> 2) + 4 (p & 3) + (s - 6)."""
    p, s = np.asarray(dev_col) // 16, np.asarray(dev_col) % 16
    return 16 * (p >> 2) + 4 * (p & 3) + (s - 6)


class Wrench:
    """Graded integer external-wrench regressor of a free-flyer model: six row blocks of ``Nb`` rows, force components
    first; 14 reference columns per link, slot s < 6 (rotational inertia) exactly zero in the three force blocks.  The
    ``n`` kept columns lie in the live links; the others are dead (all zero): the links in ``dead_links`` entirely, slots
    10 .. 13 everywhere when ``extra_slots`` is False (what the force-compact layout needs), and the rest at random (at
    least a fifth of all columns).  ``deps``: every third kept column an exact combination of earlier kept columns of its
    class (inertia / force-capable).  Attributes: M (rows x n integers over the kept columns), s (their exponents), kept
    (reference columns, ascending), link_pos (-1 for dead links), nlive, mt / st (tau: integers, exponent), dep / base
    (positions in the kept list)."""

    def __init__(self, rng, Nb, nlinks, n, lo, hi, dead_links=(), extra_slots=True, deps=False):
        self.Nb, self.nlinks, self.ncols, self.rows = Nb, nlinks, 14 * nlinks, 6 * Nb
        live = [l for l in range(nlinks) if l not in set(dead_links)]
        self.link_pos = np.full(nlinks, -1, dtype=np.int32)
        self.link_pos[live] = np.arange(len(live), dtype=np.int32)
        self.nlive = len(live)
        slots = 14 if extra_slots else 10
        cand = np.array([14 * l + s for l in live for s in range(slots)])
        assert n <= min(len(cand), int(0.8 * self.ncols)), "at least a fifth of the columns are dead"
        self.kept = np.sort(rng.choice(cand, n, replace=False))
        self.slot = self.kept % 14
        M = int_matrix(rng, self.rows, n)
        M[:3 * Nb, self.slot < 6] = 0.0
        s = graded_scales(rng, n, lo, hi, small_positions(n))
        self.dep, self.base = ([], list(range(n)))
        if deps:
            self.dep, self.base = make_dependent(rng, M, s, n, lo, same_class=(self.slot >= 6))
        self.M, self.s, self.n = M, s, n
        self.nf = int(np.count_nonzero(self.slot >= 6))
        self.mt, self.st = int_matrix(rng, self.rows, 1)[:, 0], int(rng.integers(lo, hi + 1))

    def A(self):
        """The kept columns, graded (float64, exact)."""
        return self.M * np.ldexp(1.0, self.s)

    def tau(self):
        return self.mt * 2.0 ** self.st

    def gram(self, with_tau=True):
        """Exact Gram of [W[:, kept] tau] (or of W[:, kept])."""
        if with_tau:
            return exact_gram(np.c_[self.M, self.mt], np.r_[self.s, self.st])
        return exact_gram(self.M, self.s)

    def colsq(self):
        """diag(W^T W) in the reference's numbering (zeros for the dead columns)."""
        cs = np.zeros(self.ncols)
        cs[self.kept] = np.diag(exact_gram(self.M, self.s))
        return cs

    def reference(self):
        """Reference layout: rows x 14 nlinks."""
        W = np.zeros((self.rows, self.ncols))
        W[:, self.kept] = self.A()
        return W

    def padded(self, compact=False):
        """Link-padded (16 nlinks columns) or link-compact (16 nlive columns, segment of link l at 16 link_pos[l])."""
        pos = self.link_pos if compact else None
        W = np.zeros((self.rows, 16 * (self.nlive if compact else self.nlinks)))
        W[:, device_column(self.kept, 16, pos)] = self.A()
        return W

    def force_ld(self, compact=False):
        return 16 * -(-(self.nlive if compact else self.nlinks) // 4)

    def force_compact(self, compact=False):
        """Force-compact buffer: the 3 Nb force rows over force_ld() columns (mx my mz m of link position p at
        16 (p >> 2) + 4 (p & 3) + s - 6), then the 3 Nb torque rows link-padded (or link-compact).  Returns (flat, ldw)."""
        assert not np.any(self.slot >= 10), "the force-compact layout has no slots 10 .. 13"
        half = 3 * self.Nb
        T = self.padded(compact)
        F = np.zeros((half, self.force_ld(compact)))
        fc = self.slot >= 6
        F[:, force_column(device_column(self.kept[fc], 16, self.link_pos if compact else None))] = self.A()[:half, fc]
        return np.concatenate([F.reshape(-1), T[half:].reshape(-1)]), T.shape[1]


def read_wrench_layout(buf, rows, ncols, ldw, link_stride=14, link_pos=None, ld_force=0):
    """The reference-layout W (rows x ncols) read back from a device buffer in any of the four layouts, through the
    column maps the kernels use (device_column, force_column)."""
    buf = np.asarray(buf).reshape(-1)
    c = np.arange(ncols)
    dev = device_column(c, link_stride, link_pos)
    live = np.ones(ncols, dtype=bool) if link_pos is None else np.asarray(link_pos)[c // 14] >= 0
    W = np.zeros((rows, ncols))
    if ld_force:
        half = rows // 2
        F = buf[:half * ld_force].reshape(half, ld_force)
        T = buf[half * ld_force:half * ld_force + half * ldw].reshape(half, ldw)
        fc = live & (c % 14 >= 6) & (c % 14 < 10)
        W[:half, fc] = F[:, force_column(dev[fc])]
        W[half:, live] = T[:, dev[live]]
    else:
        Wd = buf[:rows * ldw].reshape(rows, ldw)
        W[:, live] = Wd[:, dev[live]]
    return W


class RowBlocks:
    """Graded integer matrix of ``nblocks`` row blocks of ``rows_b`` rows (the joint-torque regressor of a tree): column
    groups ``groups`` = [(size, block set)], the columns of a group non-zero exactly in the rows of its blocks.  The kept
    columns are scattered over a reference space of 14 nlinks columns, a fifth of them or more dead.  ``inactive``: blocks
    whose rows hold garbage and take no part.  ``deps``: every third kept column an exact combination of earlier columns
    of its own group (its support stays in the blocks that list it).  tau = M k + e exactly: k (integers) on a few columns
    that only the block ``k_block`` lists, so phi = k 2^-s and ||tau_b - W_b phi||^2 = ||e_b||^2; ``noise`` per block: 'tiny' (+-1 in
    three rows), 'mid' (+-32), 'big' (+-2^10 in every row)."""

    def __init__(self, rng, rows_b, nblocks, groups, lo, hi, inactive=(), deps=False, noise=None, k_block=None):
        self.rows_b, self.nblocks, self.rows = rows_b, nblocks, rows_b * nblocks
        self.inactive = sorted(inactive)
        n = sum(g for g, _ in groups)
        self.n = n
        nlinks = -(-n * 5 // (4 * 14)) + 1
        self.ncols = 14 * nlinks
        self.kept = np.sort(rng.choice(self.ncols, n, replace=False))
        group = np.repeat(np.arange(len(groups)), [g for g, _ in groups])
        rng.shuffle(group)  # (the groups interleave in the kept order)
        self.group = group
        self.support = support = np.zeros((nblocks, n), dtype=bool)
        for gi, (_, blocks) in enumerate(groups):
            for b in blocks:
                support[b, group == gi] = True
        M = int_matrix(rng, self.rows, n)
        s = graded_scales(rng, n, lo, hi, small_positions(n))
        M.reshape(nblocks, rows_b, n)[~np.repeat(support[:, None, :], rows_b, axis=1)] = 0.0
        self.dep, self.base = ([], list(range(n)))
        if deps:
            self.dep, self.base = make_dependent(rng, M, s, n, lo, same_class=group)
        for b in self.inactive:  # garbage: these rows must not be read
            M[b * rows_b:(b + 1) * rows_b] = int_matrix(rng, rows_b, n)
        self.M, self.s = M, s
        self.lists = [None if b in self.inactive else np.flatnonzero(np.any(self.Mb(b) != 0, axis=0))
                      for b in range(nblocks)]
        self.counts = np.array([-1 if L is None else len(L) for L in self.lists], dtype=np.int32)
        # tau = M k + e
        k = np.zeros(n, dtype=np.int64)
        if k_block is not None:
            # (columns of that block alone: tau_b = e_b in every other block, so its residual is read without cancellation)
            alone = support.sum(axis=0) == 1
            cols = [c for c in self.lists[k_block] if c not in set(self.dep) and alone[c]]
            pick = rng.choice(cols, min(6, len(cols)), replace=False)
            k[pick] = rng.integers(1, 3, len(pick)) * rng.choice([-1, 1], len(pick))
        self.k = k
        noise = noise or {}
        e = np.zeros(self.rows)
        for b in range(nblocks):
            kind = noise.get(b, "mid")
            eb = e[b * rows_b:(b + 1) * rows_b]
            if kind == "tiny":
                eb[rng.choice(rows_b, 3, replace=False)] = rng.choice([-1.0, 1.0], 3)
            elif kind == "big":
                eb[:] = rng.choice([-1.0, 1.0], rows_b) * 2.0 ** 10
            else:
                eb[:] = rng.integers(-32, 33, rows_b)
        self.e = e
        Ma = np.where(np.isin(np.arange(self.rows) // rows_b, self.inactive)[:, None], 0.0, M)
        self.mt = Ma @ k.astype(np.float64) + e
        for b in self.inactive:
            self.mt[b * rows_b:(b + 1) * rows_b] = int_matrix(rng, rows_b, 1)[:, 0]

    def Mb(self, b):
        return self.M[b * self.rows_b:(b + 1) * self.rows_b]

    def phi(self):
        """The exact coefficients with tau = W phi + e: phi_c = k_c 2^-s_c."""
        return self.k * np.ldexp(1.0, -self.s)

    def active(self):
        return [b for b in range(self.nblocks) if b not in self.inactive]

    def block_gram(self, b, with_tau=True):
        """Exact Gram of block b's [W_b[:, list_b] tau_b] (its columns in list order, tau last)."""
        L = self.lists[b]
        Mb = self.Mb(b)[:, L]
        if with_tau:
            return exact_gram(np.c_[Mb, self.mt[b * self.rows_b:(b + 1) * self.rows_b]], np.r_[self.s[L], 0])
        return exact_gram(Mb, self.s[L])

    def gram(self, with_tau=True, cols=None, block_exp=None):
        """Gram of the active rows of [W[:, kept] tau] (columns ``cols`` of it, tau = position n), the blocks' rows scaled
        by 2^block_exp[b]: the long-double sum of the exact per-block Grams (column-wise error <= 2^-64 |a_i| |a_j|)."""
        check_longdouble()
        nc = self.n + (1 if with_tau else 0)
        cols = np.arange(nc) if cols is None else np.asarray(cols)
        G = np.zeros((len(cols), len(cols)), dtype=np.longdouble)
        for b in self.active():
            sl = slice(b * self.rows_b, (b + 1) * self.rows_b)
            X = np.c_[self.M[sl], self.mt[sl]] if with_tau else self.M[sl]
            sx = np.r_[self.s, 0] if with_tau else self.s
            Gb = exact_gram(X[:, cols], sx[cols])
            if block_exp is not None:
                Gb = Gb * 4.0 ** float(block_exp[b])
            G += np.asarray(Gb, dtype=np.longdouble)
        return G

    def tau(self):
        return self.mt

    def colsq(self):
        active = ~np.isin(np.arange(self.rows) // self.rows_b, self.inactive)
        cs = np.zeros(self.ncols)
        cs[self.kept] = (self.M[active] ** 2).sum(axis=0) * np.ldexp(1.0, 2 * self.s)  # (exact: integers below 2^53)
        return cs

    def A(self):
        return self.M * np.ldexp(1.0, self.s)

    def dense(self, link_stride=16):
        """Dense W in the device numbering (reference layout for stride 14, link-padded for 16)."""
        W = np.zeros((self.rows, (self.ncols // 14) * link_stride))
        W[:, device_column(self.kept, link_stride)] = self.A()
        return W

    def block_columns(self, link_stride=16):
        """(counts, cols, pos) for the dense W: per active block its list, as device columns and kept positions."""
        cols = np.concatenate([device_column(self.kept[L], link_stride) for L in self.lists if L is not None] + [[0]])
        pos = np.concatenate([L for L in self.lists if L is not None] + [[0]])
        return self.counts, cols.astype(np.int32), pos.astype(np.int32)

    def compact(self, link_stride=16):
        """Block-compact W: block b is its own rows_b x ld_b matrix (the window of links its list spans, 16 columns per
        link; nothing for an inactive block).  Returns (flat, offsets, lds, local cols)."""
        parts, off, lds, cols, at = [], [], [], [], 0
        A = self.A()
        for b in range(self.nblocks):
            L = self.lists[b]
            if L is None or len(L) == 0:
                off.append(at)
                lds.append(0)
                continue
            dev = device_column(self.kept[L], 16)
            first = int(dev.min()) // 16
            ld = 16 * (int(dev.max()) // 16 - first + 1)
            Wb = np.zeros((self.rows_b, ld))
            local = dev - 16 * first
            Wb[:, local] = A[b * self.rows_b:(b + 1) * self.rows_b][:, L]
            parts.append(Wb.reshape(-1))
            off.append(at)
            lds.append(ld)
            cols.append(local)
            at += Wb.size
        flat = np.concatenate(parts) if parts else np.zeros(1)
        return flat, np.asarray(off, dtype=np.int64), np.asarray(lds, dtype=np.int32), \
            np.concatenate(cols + [[0]]).astype(np.int32)

    def stack_offsets(self, with_tau=True):
        """Row offsets of the blocks in the compact stack: n_j (+ 1) rows per block that has any, none otherwise."""
        rows = [0 if (c < 0 or (c == 0 and not with_tau)) else c + (1 if with_tau else 0) for c in self.counts]
        return np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)


def residual_ratio(r2, e2, v, Gb):
    """|r2 - e2| / (u (sum_c |v_c| |a_c|)^2), |a_c| the column norms of the block Gram ``Gb``: the column-wise backward
    bound of v^T (S^T S) v, for a block residual r2 whose exact value is e2."""
    a = np.sqrt(np.diag(np.asarray(Gb, dtype=np.float64)))
    return abs(float(r2) - float(e2)) / (2.0 ** -53 * float((np.abs(np.asarray(v)) * a).sum()) ** 2)
