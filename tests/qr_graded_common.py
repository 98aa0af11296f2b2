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
