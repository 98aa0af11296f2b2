"""References for the singular-value tests (test_singular_values_host.py, test_singular_values_entrywise.py).

The test matrices: for every r of ``SIZES`` and every ratio of ``RATIOS`` the triangle R of a (4 r + 3) x r matrix whose
singular values are graded logarithmically over that ratio and whose columns are then scaled by a permutation of
``logspace(-2, 2, r)`` -- regressor columns differ like that (inertias against first moments against friction).  The strict
lower triangle is NaN wherever a matrix is handed to code under test: nothing may read it.

The reference of a matrix is the package's own one-sided Jacobi mirror (_host.jacobi_singular_values_mirror) run in
``np.longdouble`` (64-bit mantissa), sorted.  The bound on a float64 result is

    |sigma_k - ref_k| <= C r 2^-53 sigma_max

C_ORACLE is the largest such ratio of the float64 mirror over all matrices below, measured by the host test
(test_c_oracle_matches_the_recorded_figures); C_SV, what a float64 kernel may use, is the power of two in [8, 16] x C_ORACLE
(the project's rule: other summation orders and contracted operations stay within it).  A device result is compared with the
long-double reference, whose own error is 2^-11 of a float64's: the device bound is C_SV (1 - 2^-11).

``jacobi_scalar`` is the same algorithm written a second time, pair by pair in scalar loops with plain dot products: the
planted errors of the host test are planted there."""
import functools

import numpy as np

SIZES = (1, 2, 3, 15, 16, 17, 40, 63, 64, 65, 98, 127, 128)
RATIOS = (1.0, 1e3, 1e6)
EPS = 2.0 ** -53
SENTINEL = -7.25e77
MAX_SWEEPS = 40

C_ORACLE = 1.652  # measured: r = 128, ratio 1e6 (LAPACK's dgesdd on the same matrices and the same scale: 0.02 .. 0.82)
C_SV = 16.0  # the power of two in [8, 16] x C_ORACLE
SWEEPS_SEEN = 22  # the most sweeps the float64 mirror needs on these matrices (r = 127 and 128, ratio 1e6); MAX_SWEEPS is 40


@functools.lru_cache(maxsize=None)
def matrix(r, ratio, seed=0):
    """The r x r upper triangle (strict lower part zero) described above; read-only."""
    from figaroh_plus_amd._host import single_threaded_blas
    rng = np.random.default_rng(1000 * r + int(np.log10(ratio)) + 7919 * seed)
    m = 4 * r + 3
    with single_threaded_blas():  # (the bits of the matrices do not depend on how many threads the host has)
        U = np.linalg.qr(rng.normal(size=(m, r)))[0]
        V = np.linalg.qr(rng.normal(size=(r, r)))[0]
        s = np.logspace(0.0, -np.log10(ratio), r) if r > 1 else np.ones(1)
        A = (U * s) @ V.T
        A = A * rng.permutation(np.logspace(-2.0, 2.0, r))
        R = np.triu(np.linalg.qr(A)[1])
    R.setflags(write=False)
    return R


def with_nan_below(R):
    """A copy whose strict lower triangle is NaN."""
    R = np.array(R, dtype=np.float64)
    R[..., np.tril_indices(R.shape[-1], -1)[0], np.tril_indices(R.shape[-1], -1)[1]] = np.nan
    return R


def cases():
    return [(r, ratio) for r in SIZES for ratio in RATIOS] + [(r, CLOSE) for r in (3, 17)]


CLOSE = "close_pair"  # in place of a ratio: the matrix of close_pair(r)


def close_pair(r):
    """Two columns of equal norm whose cosine is 2^-30, the others orthogonal to them: the singular values of the pair are
    1 -+ 2^-31 to first order, so a pair that is skipped although its cosine is far above 2^-52 shows in sigma itself."""
    R = np.diag(np.concatenate(([1.0, 1.0], np.logspace(0.5, -2.0, max(r - 2, 1))[:r - 2])))
    R[0, 1] = 2.0 ** -30
    R.setflags(write=False)
    return R


def matrix_of(r, ratio):
    return close_pair(r) if ratio == CLOSE else matrix(r, ratio)


@functools.lru_cache(maxsize=None)
def _references(r):
    """Long-double singular values, sorted (descending), of every matrix of size r in one batched run of the mirror."""
    from figaroh_plus_amd._host import jacobi_singular_values_mirror
    kinds = RATIOS + ((CLOSE,) if r >= 2 else ())
    s, _, conv = jacobi_singular_values_mirror(with_nan_below(np.stack([matrix_of(r, k) for k in kinds])), max_sweeps=60,
                                               dtype=np.longdouble)
    assert conv.all()
    ref = -np.sort(-s, axis=1)
    ref.setflags(write=False)
    return dict(zip(kinds, ref))


def reference(r, ratio):
    """Sorted (descending) long-double singular values of matrix_of(r, ratio); read-only, computed once per size."""
    return _references(r)[ratio]


def ratio_to_reference(sigma, ref):
    """max_k |sigma_k - ref_k| / (r 2^-53 sigma_max) with sigma sorted descending first."""
    sigma = -np.sort(-np.asarray(sigma, dtype=np.longdouble))
    r = len(ref)
    return float(np.abs(sigma - ref).max() / (r * np.longdouble(EPS) * ref[0]))


def jacobi_scalar(R, max_sweeps=MAX_SWEEPS, plant=None):
    """(sigma, sweeps, converged) of ONE r x r matrix, pair by pair.  ``plant``: "last_step" (the last step of every sweep is
    dropped), "sign" (the sign of t flipped), "lower" (the whole matrix is read, not its upper triangle), "threshold" (pairs
    are skipped below 2^-26 instead of 2^-52)."""
    from figaroh_plus_amd._host import jacobi_round_robin
    R = np.asarray(R, dtype=np.float64)
    r = R.shape[0]
    A = np.array(R if plant == "lower" else np.triu(R))
    steps = jacobi_round_robin(r)
    if plant == "last_step":
        steps = steps[:-1]
    thr = 2.0 ** (-26 if plant == "threshold" else -52)
    with np.errstate(all="ignore"):
        for w in range(max_sweeps):
            rotated = False
            for ps, qs in steps:
                for p, q in zip(ps, qs):
                    ap, aq = A[:, p].copy(), A[:, q].copy()
                    alpha, beta, gamma = float(ap @ ap), float(aq @ aq), float(ap @ aq)
                    if abs(gamma) <= thr * np.sqrt(alpha * beta):
                        continue
                    zeta = (beta - alpha) / (2.0 * gamma)
                    t = (-1.0 if zeta < 0 else 1.0) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                    if plant == "sign":
                        t = -t
                    c = 1.0 / np.sqrt(1.0 + t * t)
                    s = c * t
                    A[:, p], A[:, q] = c * ap - s * aq, s * ap + c * aq
                    rotated = True
            if not rotated:
                return np.sqrt((A * A).sum(axis=0)), w + 1, 1
    return np.sqrt((A * A).sum(axis=0)), max_sweeps, 0


def special_cases():
    """{tag: R} of the special matrices (r = 3, the identity r = 5) that the mirror and the kernel are both asked."""
    zero_col = np.triu(np.arange(1.0, 10.0).reshape(3, 3))
    zero_col[:, 1] = 0.0
    nan = np.triu(np.arange(1.0, 10.0).reshape(3, 3))
    nan[0, 2] = np.nan
    return {"zero": np.zeros((3, 3)), "zero_column": zero_col, "identity": np.eye(5), "nan": nan}
