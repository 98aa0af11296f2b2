"""References and bounds for the column-norm and residual-sum tests (tests/test_reductions_graded.py, the helper tests in
test_host_logic.py).

The elimination (regressor.py:271, ``col_norm[i] < tol_e``) compares a squared column norm with an ABSOLUTE threshold, and
the WLS weights are 1 / sigma_j of every joint.  The suite's older checks divide by the largest column norm (or the largest
variance); these helpers give per-column and per-joint references instead:

* ``colsq_ld``: sum_i W_ij^2 in np.longdouble, in row chunks (host memory stays bounded at 10^6 samples);
* ``gamma``: gamma_m = m u / (1 - m u), the a-priori relative bound of ANY summation order of m nonnegative rounded
  squares, with or without FMA contraction (Higham, Accuracy and Stability, Lemma 3.1 / 3.3);
* ``colsq_ratio``: the per-column error against that bound (zero columns must come out exactly zero);
* ``scale_to_norm``: an input column scaled so that the long-double sum of squares of its float64 values lands on a
  claimed side of a threshold, with a claimed margin -- the columns of the regressor that are copies of an input (the
  actuator-inertia column is a column of ``a``, the viscous-friction column one of ``v``) then straddle ``tol_e``;
* ``sigma2_direct_bound``: the a-priori bound of a per-joint variance formed from y = W_b phi and ||tau_j - y_j||^2.
"""
import numpy as np

U = 2.0 ** -53
ROW_CHUNK = 100000


def gamma(m):
    """gamma_m = m u / (1 - m u) (u = 2^-53)."""
    mu = float(m) * U
    assert mu < 0.5
    return mu / (1.0 - mu)


def colsq_ld(W, chunk=ROW_CHUNK):
    """Column sums of squares of the float64 matrix ``W`` in np.longdouble, ``chunk`` rows at a time.  The squares and the
    sums are rounded to 64 bits: relative error <= m 2^-64 per column, far below the gamma_m of float64."""
    W = np.asarray(W)
    out = np.zeros(W.shape[1], dtype=np.longdouble)
    for r0 in range(0, W.shape[0], chunk):
        X = np.asarray(W[r0:r0 + chunk], dtype=np.longdouble)
        out += (X * X).sum(axis=0)
    return out


def exact_colsq(M, s):
    """diag of the exact Gram of ``M * 2^s`` (integer M, power-of-two column scales), from int64 sums: exact as long as
    every column's integer sum stays below 2^53 (asserted)."""
    Mi = np.asarray(M).astype(np.int64)
    assert np.array_equal(Mi, M)
    tot = (Mi * Mi).sum(axis=0)
    assert tot.max(initial=0) < 2 ** 53
    return tot.astype(np.float64) * np.ldexp(1.0, 2 * np.asarray(s, dtype=np.int64))


def colsq_ratio(cs, ref, m, slack=0.0):
    """Per-column relative error of ``cs`` against the long-double ``ref`` divided by gamma_m + slack.  A column whose
    reference is exactly zero must be exactly zero (ratio inf otherwise).  Returns the array of ratios."""
    cs = np.asarray(cs, dtype=np.longdouble)
    ref = np.asarray(ref, dtype=np.longdouble)
    bound = gamma(m) + slack
    zero = ref == 0
    r = np.zeros(len(ref))
    r[zero] = np.where(cs[zero] == 0, 0.0, np.inf)
    nz = ~zero
    r[nz] = np.asarray(np.abs(cs[nz] - ref[nz]) / ref[nz], dtype=np.float64) / bound
    return r


def colsq_worst_over_log_u(cs, ref, m):
    """max_j e_j / (log2(m) u), e_j the relative error of column j (what the tests record)."""
    cs = np.asarray(cs, dtype=np.longdouble)
    ref = np.asarray(ref, dtype=np.longdouble)
    nz = ref != 0
    if not nz.any():
        return 0.0
    e = np.asarray(np.abs(cs[nz] - ref[nz]) / ref[nz], dtype=np.float64)
    return float(e.max()) / (max(1.0, np.log2(max(m, 2))) * U)


def normwise_colsq_ok(cs, ref, rel=1e-12):
    """The suite's older check: |cs - ref| <= rel * max(ref) for every column."""
    ref = np.asarray(ref, dtype=np.float64)
    return bool((np.abs(np.asarray(cs, dtype=np.float64) - ref) <= rel * ref.max()).all())


def exact_split(ref, tol_e):
    """(idx_e, kept) of the elimination on the exact norms: idx_e = {j : ref_j < tol_e}."""
    ref = np.asarray(ref, dtype=np.longdouble)
    e = ref < tol_e
    return np.flatnonzero(e).tolist(), np.flatnonzero(~e).tolist()


def undecided(ref, tol_e, band):
    """Columns whose exact norm lies within tol_e * [1 - band, 1 + band]: a correct kernel may put them on either side."""
    ref = np.asarray(ref, dtype=np.longdouble)
    lo, hi = np.longdouble(tol_e) * (1 - np.longdouble(band)), np.longdouble(tol_e) * (1 + np.longdouble(band))
    return np.flatnonzero((ref >= lo) & (ref <= hi)).tolist()


def scale_to_norm(x, target, factor=1):
    """``x`` (float64 vector, not all zero) scaled so that ``factor`` * sum(y^2), summed in long double over the float64
    values y, is ``target`` up to a few u.  ``factor``: the number of rows a copied input lands on per sample (six in the
    external-wrench mode).  Returns (y, achieved)."""
    x = np.asarray(x, dtype=np.float64)
    s0 = factor * float(colsq_ld(x.reshape(-1, 1))[0])
    y = x * np.sqrt(float(target) / s0)
    return y, factor * colsq_ld(y.reshape(-1, 1))[0]


def straddle(x, tol_e, side, margin=1e-9, factor=1):
    """``x`` scaled to tol_e (1 + side margin) (side = +1 above, -1 below).  Asserts that the long-double sum of squares of
    the float64 result lies on that side of tol_e by at least 0.99 margin."""
    y, got = scale_to_norm(x, tol_e * (1.0 + side * margin), factor)
    rel = (got - np.longdouble(tol_e)) / np.longdouble(tol_e)
    assert side * rel >= 0.99 * margin, "straddle: %.3e" % float(rel)
    return y, got


def sigma2_ld(tau, y, n_j):
    """Long-double ||tau_j - y_j||^2 / n_j per block (``n_j``: the block lengths, consecutive)."""
    out, off = [], 0
    for n in n_j:
        d = np.asarray(tau[off:off + n], dtype=np.longdouble) - np.asarray(y[off:off + n], dtype=np.longdouble)
        out.append((d * d).sum() / n)
        off += n
    return np.array(out, dtype=np.longdouble)


def sigma2_direct_bound(tau, Wb, phi, n_j, r_norm):
    """A-priori bound of n_j |sigma2_j - sigma2*_j| for sigma2 formed as ||tau_j - fl(W_b phi)_j||^2 in float64:
    2 ||r_j|| ||e_j|| + ||e_j||^2 + gamma_{n_j} ||r_j||^2 with |e_i| <= gamma_{n+2} (|tau_i| + sum_c |W_ic phi_c|)
    (the dot product of n terms, the subtraction, the square).  ``r_norm``: the exact ||r_j||.  Returns one bound per
    block, divided by n_j (the bound on sigma2 itself)."""
    n = Wb.shape[1]
    E = gamma(n + 2) * (np.abs(np.asarray(tau, dtype=np.longdouble))
                        + np.abs(np.asarray(Wb, dtype=np.longdouble)) @ np.abs(np.asarray(phi, dtype=np.longdouble)))
    out, off = [], 0
    for j, nb in enumerate(n_j):
        e = np.sqrt((E[off:off + nb] ** 2).sum())
        r = np.longdouble(r_norm[j])
        out.append((2 * r * e + e * e + gamma(nb) * r * r) / nb)
        off += nb
    return np.array(out, dtype=np.longdouble)


def sigma2_triangle_bounds(A_norms, v, r_norm, nc, n_j, tol_backward):
    """Bounds of the per-row-block triangle path (figh_block_rows_residuals on a triangle S_j of [W_j tau_j]):
    (tight, loose).  tight: e = tol_backward sum_c ||a_{j,c}|| |v_c| in place of ||e_j|| in the direct bound, plus the
    residual kernel's own gamma_{nc} ||r_j||^2 -- it assumes a column-wise backward error of the triangle.  loose: what
    the Gram metric alone implies, tol_backward (sum_c ||a_{j,c}|| |v_c|)^2.  Both divided by n_j."""
    tight, loose = [], []
    for j, nb in enumerate(n_j):
        s = float(np.dot(np.asarray(A_norms[j], dtype=np.float64), np.abs(np.asarray(v, dtype=np.float64))))
        e = tol_backward * s
        r = float(r_norm[j])
        tight.append((2 * r * e + e * e + (gamma(nb) + gamma(nc)) * r * r) / nb)
        loose.append(tol_backward * s * s / nb)
    return np.array(tight), np.array(loose)
