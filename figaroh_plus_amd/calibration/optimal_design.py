"""D-optimal selection of calibration postures (``examples/tiago/optimal_config.py``, ``examples/ur10/optimal_config.py``)
on two data-parallel passes over the base kinematic regressor of a pool of candidate postures.

The reference cuts ``R_b`` into one ``calibration_index x n`` block per posture, stores every information matrix
``X_i = R_i^T R_i`` (``sub_info_matrix``, ``:42-60``) and hands them to picos / cvxopt (``SOCP``, ``:129-160``) or to the
``Detmax`` exchange loop (``:63-126``), one ``n x n`` determinant per candidate and step.  Here nothing per candidate is
stored.  With ``M(w) = sum_i w_i X_i`` and ``G_i = R_i M^-1 R_i^T`` (``c x c``, ``c = calibration_index``):

* ``tr G_i = d_i`` is the variance function; ``w_i <- w_i d_i / n`` ascends ``log det M(w)`` on the simplex and
  ``max_i d_i <= n (1 + eps)`` certifies D-efficiency ``>= 1 / (1 + eps)`` (Kiefer-Wolfowitz equivalence theorem);
* ``det(I + G_i) = det(M + X_i) / det M`` and ``det(I - G_i) = det(M - X_i) / det M`` are Detmax's add and remove scores.

``figh_design_gram`` and ``figh_design_scores`` (csrc/figh_design.hip) run the passes on the device over a resident
``GpuMatrix`` in the layout ``calculate_base_kinematics_regressor`` leaves (row ``k N + i``: component ``k`` of posture
``i``); ``gram_mirror`` and ``scores_mirror`` are the float64 NumPy mirrors, the second one in the kernel's operation order
(bit-equal).  Without a device the mirrors run.

Out of scope: the posture YAML files, plots, A- / C-optimality, shrinking the pool during the solve.
"""
import numpy as np

from .. import _lib
from ..device import GpuMatrix

MAX_COLS = 96   # include/figh.h FIGH_DESIGN_MAX_COLS
MAX_COMPONENTS = 6


# ------------------------------------------------------------------------------------------- the reference's two helpers
def rearrange_rb(R_b, param):
    """``R_b`` (row ``k NbSample + i``) reordered by sample (row ``i calibration_index + k``), optimal_config.py:31-39."""
    R_b = np.asarray(R_b)
    c, N = int(param["calibration_index"]), int(param["NbSample"])
    out = np.empty_like(R_b)
    out[:c * N] = R_b[:c * N].reshape(c, N, -1).transpose(1, 0, 2).reshape(c * N, -1)
    return out


def sub_info_matrix(R, param):
    """``(subX_list, subX_dict)``: ``X_i = R_i^T R_i`` of the ``calibration_index`` rows of every sample in the rearranged
    regressor (optimal_config.py:42-60), as one batched product."""
    c, N = int(param["calibration_index"]), int(param["NbSample"])
    blocks = np.asarray(R, dtype=np.float64)[:c * N].reshape(N, c, -1)
    X = np.matmul(blocks.transpose(0, 2, 1), blocks)
    subX_list = [X[i] for i in range(N)]
    return subX_list, dict(zip(np.arange(N), subX_list))


# -------------------------------------------------------------------------------------------------------------- mirrors
def gram_mirror(R, N, c, w=None):
    """``M = sum_i w_i sum_k r_{k,i} r_{k,i}^T`` of the component-major ``R`` (``c N x n``), exactly symmetric."""
    R = np.asarray(R, dtype=np.float64)
    n = R.shape[1]
    M = np.zeros((n, n))
    for k in range(c):
        Rk = R[k * N:(k + 1) * N]
        M += (Rk if w is None else Rk * np.asarray(w, dtype=np.float64)[:, None]).T @ Rk
    low = np.tril(M)
    return low + np.tril(M, -1).T


def _pivots_product(G, c, minus):
    """Product of the pivots of the symmetric elimination of I + G / I - G in the order of csrc/figh_design.hip."""
    A = {}
    for p in range(c):
        for q in range(p, c):
            if p == q:
                A[p, q] = (1.0 - G[p, p]) if minus else (1.0 + G[p, p])
            else:
                A[p, q] = -G[p, q] if minus else G[p, q].copy()
    det = np.ones_like(G[0, 0])
    ok = np.ones(det.shape, dtype=bool)
    for p in range(c):
        piv = A[p, p]
        if minus:
            ok &= piv > 0.0
        det = det * piv
        for r in range(p + 1, c):
            f = A[p, r] / piv
            for q in range(r, c):
                A[r, q] = A[r, q] - f * A[p, q]
    return np.where(ok, det, 0.0) if minus else det


def scores_mirror(R, N, c, L, want=(True, True, True)):
    """``(tr G_i, det(I + G_i), det(I - G_i))`` for every candidate in the operation order the header comment of
    csrc/figh_design.hip fixes -- one correctly rounded operation per NumPy operation, so the device gives the same bits.
    ``want``: which of the three to form (None in place of the others)."""
    R = np.asarray(R, dtype=np.float64)
    L = np.asarray(L, dtype=np.float64)
    n = R.shape[1]
    Y = np.empty((n, c * N))
    with np.errstate(all="ignore"):
        for a in range(n):
            s = R[:c * N, a].copy()
            for b in range(a):
                s = s - L[a, b] * Y[b]
            Y[a] = s / L[a, a]
        G = {}
        for k in range(c):
            for l in range(k, c):
                g = np.zeros(N)
                for a in range(n):
                    g = g + Y[a, k * N:(k + 1) * N] * Y[a, l * N:(l + 1) * N]
                G[k, l] = g
        t = np.zeros(N)
        for k in range(c):
            t = t + G[k, k]
        return (t if want[0] else None, _pivots_product(G, c, False) if want[1] else None,
                _pivots_product(G, c, True) if want[2] else None)


# ----------------------------------------------------------------------------------------------------------------- pool
class CandidatePool:
    """The base kinematic regressor of ``NbSample`` candidate postures, ``calibration_index`` measured components each, in
    the component-major layout: an ndarray or a ``GpuMatrix`` (which stays resident and is never downloaded).  With a device
    a host array is uploaded once and both passes run there; without one the mirrors run."""

    def __init__(self, R_b, NbSample, calibration_index):
        self.N, self.c = int(NbSample), int(calibration_index)
        rows, cols = R_b.shape
        if not 1 <= self.c <= MAX_COMPONENTS or self.N < 1:
            raise ValueError("calibration_index must lie in 1 .. %d and NbSample be positive" % MAX_COMPONENTS)
        if rows != self.c * self.N:
            raise ValueError("R_b has %d rows, calibration_index x NbSample = %d x %d = %d: rows were deleted (2-norm below "
                             "1e-6) and the blocks of a posture no longer line up" % (rows, self.c, self.N, self.c * self.N))
        if not 1 <= cols <= MAX_COLS:
            raise ValueError("R_b has %d columns, the design passes take 1 .. %d" % (cols, MAX_COLS))
        self.n = int(cols)
        self.R_dev = self.R_host = None
        if isinstance(R_b, GpuMatrix):
            self.R_dev = R_b
        elif _lib.device_count() > 0:
            self.R_dev = GpuMatrix.from_host(R_b)
        else:
            self.R_host = np.ascontiguousarray(R_b, dtype=np.float64)
        self._out = None

    @property
    def on_device(self):
        return self.R_dev is not None

    def keys(self):
        return range(self.N)

    def information_matrix(self, w=None):
        """``M(w) = sum_i w_i X_i`` (``w = None``: all ones), an exactly symmetric (n, n) host array."""
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
            if w.size != self.N:
                raise ValueError("%d weights for %d candidates" % (w.size, self.N))
        if not self.on_device:
            return gram_mirror(self.R_host, self.N, self.c, w)
        d_w = _lib.DeviceArray.from_host(w) if w is not None else None
        return _lib.design_gram(self.R_dev.ptr, self.R_dev.ld, self.N, self.c, self.n, d_w)

    def subset_information_matrix(self, indices):
        """``sum_{i in indices} X_i``; an index listed several times counts that often."""
        idx = np.asarray(list(indices), dtype=np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= self.N):
            raise ValueError("chosen sample not in candidate pool")
        return self.information_matrix(np.bincount(idx, minlength=self.N).astype(np.float64))

    def scores(self, M, want=(True, True, True)):
        """``(d, det_add, det_rm)`` of every candidate against ``M``: ``tr G_i``, ``det(I + G_i)``, ``det(I - G_i)`` (+0.0
        where ``M - X_i`` is not positive definite).  ``numpy.linalg.LinAlgError`` when ``M`` is not positive definite.
        ``want``: which of the three are formed and brought to the host (None in place of the others)."""
        L = np.linalg.cholesky(np.asarray(M, dtype=np.float64))
        if not self.on_device:
            return scores_mirror(self.R_host, self.N, self.c, L, want)
        if self._out is None:
            self._out = [_lib.DeviceArray((self.N,)) for _ in range(3)]
        outs = [o if on else None for o, on in zip(self._out, want)]
        _lib.design_scores(self.R_dev.ptr, self.R_dev.ld, self.N, self.c, self.n, L, *outs)
        return tuple(o.to_host() if o is not None else None for o in outs)


class _MatrixPool:
    """The reference's ``subX_dict`` behind the two methods the solvers use (host only: the X_i are already formed)."""

    def __init__(self, subX_dict):
        self.index = list(subX_dict.keys())
        self.X = np.stack([np.asarray(subX_dict[i], dtype=np.float64) for i in self.index])
        self.N, self.n = self.X.shape[0], self.X.shape[1]

    def keys(self):
        return self.index

    def information_matrix(self, w=None):
        M = self.X.sum(axis=0) if w is None else np.tensordot(np.asarray(w, dtype=np.float64), self.X, axes=1)
        return np.tril(M) + np.tril(M, -1).T

    def subset_information_matrix(self, indices):
        pos = {key: p for p, key in enumerate(self.index)}
        assert all(i in pos for i in indices), "chosen sample not in candidate pool"
        return self.information_matrix(np.bincount([pos[i] for i in indices], minlength=self.N).astype(np.float64))

    def scores(self, M, want=(True, True, True)):
        L = np.linalg.cholesky(np.asarray(M, dtype=np.float64))  # (raises unless M is positive definite)
        Minv = np.linalg.inv(L).T @ np.linalg.inv(L)
        d = np.einsum("ab,iba->i", Minv, self.X)
        sign_a, logdet_a = np.linalg.slogdet(M + self.X)
        sign_r, logdet_r = np.linalg.slogdet(M - self.X)
        _, logdet = np.linalg.slogdet(M)
        return d, sign_a * np.exp(logdet_a - logdet), np.where(sign_r > 0, np.exp(logdet_r - logdet), 0.0)


def _as_pool(pool):
    return pool if hasattr(pool, "information_matrix") else _MatrixPool(pool)


def _det_root(M):
    """``det(M)^(1/n)`` (picos ``DetRootN``) through the Cholesky factor; 0.0 when M is not positive definite."""
    try:
        diag = np.diag(np.linalg.cholesky(M))
    except np.linalg.LinAlgError:
        return 0.0
    return float(np.exp(2.0 * np.sum(np.log(diag)) / M.shape[0]))


# -------------------------------------------------------------------------------------------------------------- solvers
class SOCP:
    """The programme of optimal_config.py:129-160 -- maximise ``t <= DetRootN(sum_i w_i X_i)`` subject to ``sum w <= 1``,
    ``w >= 0`` -- solved by another algorithm: the multiplicative update ``w_i <- w_i d_i / n`` from uniform weights, whose
    fixed point is the same optimum (the constraint ``sum w <= 1`` is active at it and the update keeps ``sum w = 1``).  The
    weights agree with an interior-point solution in the value of the criterion, within the certified efficiency bound,
    not digit for digit: the optimal weights need not be unique when the X_i are linearly dependent.

    ``pool``: a ``CandidatePool`` or the reference's ``subX_dict``.  After ``solve``: ``iterations``, ``max_variance``
    (``max_i d_i``) and ``efficiency_bound = n / max_i d_i``."""

    def __init__(self, pool, param):
        self.pool = _as_pool(pool)
        self.param = param
        if int(param["NbSample"]) != self.pool.N:
            raise ValueError("param[\"NbSample\"] = %d, the pool holds %d candidates" % (int(param["NbSample"]), self.pool.N))
        self.iterations, self.max_variance, self.efficiency_bound = 0, None, None

    def solve(self, tol=1e-3, max_iter=10000):
        """``(w_list, w_dict_sort)`` as the reference returns them.  Stops when ``max_i d_i <= n (1 + tol)``; RuntimeError
        when ``max_iter`` updates do not get there."""
        N, n = self.pool.N, self.pool.n
        w = np.full(N, 1.0 / N)
        for it in range(max_iter + 1):
            d = self.pool.scores(self.pool.information_matrix(w), want=(True, False, False))[0]
            self.iterations, self.max_variance = it, float(d.max())
            self.efficiency_bound = n / self.max_variance
            if self.max_variance <= n * (1.0 + tol):
                break
            if it == max_iter:
                raise RuntimeError("SOCP.solve: max d / n = %.6g after %d updates, above 1 + tol = %.6g"
                                   % (self.max_variance / n, max_iter, 1.0 + tol))
            w = w * d / n
        self.w = w
        w_list = [float(x) for x in w]
        print("sum of all element in vector solution: ", sum(w_list))
        w_dict = dict(zip(np.arange(N), w_list))
        w_dict_sort = dict(reversed(sorted(w_dict.items(), key=lambda item: item[1])))
        return w_list, w_dict_sort


class Detmax:
    """The exchange loop of optimal_config.py:63-126 on the two passes: a step is two Gram passes and two scores passes
    instead of one ``n x n`` determinant per candidate."""

    def __init__(self, candidate_pool, NbChosen):
        self.pool = _as_pool(candidate_pool)
        self.nd = int(NbChosen)
        self.cur_set = []
        self.fail_set = []
        self.opt_set = []
        self.opt_critD = []

    def get_critD(self, set):
        """``DetRootN`` of the information matrix of the listed candidates (:72-80)."""
        return _det_root(self.pool.subset_information_matrix(set))

    def main_algo(self, initial_set=None, rng=None):
        """The reference loop, statement by statement; returns the list of criteria and fills ``opt_set``.  ``initial_set``
        replaces the random start (``random.sample``), which is otherwise drawn from ``numpy.random.default_rng(rng)``."""
        n = self.pool.n
        pool_idx = list(self.pool.keys())
        if initial_set is None:
            cur_set = [pool_idx[p] for p in np.random.default_rng(rng).choice(len(pool_idx), self.nd, replace=False)]
        else:
            cur_set = list(initial_set)
        # (the reference subtracts the EMPTY self.cur_set: the add scan covers the whole pool)
        updated_pool = pool_idx
        opt_k = updated_pool[0]
        opt_critD = self.get_critD(cur_set)
        rm_j = cur_set[0]
        pos = {key: p for p, key in enumerate(pool_idx)}
        while opt_k != rm_j:
            # add: the first candidate whose criterion is strictly above everything before it
            M = self.pool.subset_information_matrix(cur_set)
            root = _det_root(M)
            crit = root * self.pool.scores(M, want=(False, True, False))[1] ** (1.0 / n)
            best = int(np.argmax(crit))
            if opt_critD < crit[best]:
                opt_k = updated_pool[best]
            # (the scan's ``cur_set.append(k)`` ... ``cur_set.remove(k)`` takes out the FIRST k: a member the scan passes
            # moves to the end of the list, which decides later ties and the default ``rm_j = cur_set[0]``)
            for k in sorted(set(cur_set), key=pos.__getitem__):
                cur_set.remove(k)
                cur_set.append(k)
            cur_set.append(opt_k)
            # remove: the first member whose removal loses strictly less than everything before it
            M = self.pool.subset_information_matrix(cur_set)
            opt_critD = _det_root(M)
            det_rm = self.pool.scores(M, want=(False, False, True))[2]
            loss = opt_critD - opt_critD * det_rm[[pos[j] for j in cur_set]] ** (1.0 / n)
            least = int(np.argmin(loss))
            rm_j = cur_set[least] if loss[least] < opt_critD else cur_set[0]
            cur_set.remove(rm_j)
            opt_critD = self.get_critD(cur_set)
            self.opt_critD.append(opt_critD)
        self.cur_set = list(cur_set)
        self.opt_set = list(cur_set)
        return self.opt_critD


# -------------------------------------------------------------------------------------------------- around the solvers
def detroot_whole(pool):
    """``DetRootN(R^T R) / sqrt(n)`` of the whole pool (optimal_config.py:257-264)."""
    M = _as_pool(pool).information_matrix(None)
    return _det_root(M) / np.sqrt(M.shape[0])


def minNbChosen(param):
    """The least number of postures a design needs (optimal_config.py:171-184)."""
    if param["calib_model"] == "full_params":
        return int(len(param["actJoint_idx"]) * 6 / param["calibration_index"]) + 1
    if param["calib_model"] == "joint_offset":
        return int(len(param["actJoint_idx"]) / param["calibration_index"]) + 1
    assert False, "Calibration model not supported."


def select_configurations(w_dict_sort, eps_opt=1e-5, min_chosen=0):
    """The candidates whose weight exceeds ``eps_opt``, heaviest first, and the reference's feasibility assertion
    (optimal_config.py:279-290); ``min_chosen``: ``minNbChosen(param)``."""
    chosen_config = [i for i in w_dict_sort if w_dict_sort[i] > eps_opt]
    assert len(chosen_config) >= min_chosen, "Infeasible design, try to increase NbSample."
    return chosen_config
