"""Shared by the posture-selection tests (tests/test_design_host.py, tests/test_design_entrywise.py): the pool fixture as a
base kinematic regressor, small random problems with graded columns, the exact restatement (integer arithmetic for the
Gram matrix, mpmath at 50 digits for the scores), the derived bounds, and a copy of the mirrors that takes planted errors.

The bounds (u = 2^-53):
  Gram     |M_ab - exact| <= (c N + 2) u S_ab, S_ab = sum_i w_i sum_k |r_a| |r_b|: c N products, each rounded once together with
           its weight (two roundings), summed in any order.
  scores   kappa = cond_2(L).  Forward substitution solves (L + dL) y = r with |dL| <= n u |L| row by row, so the relative
           error of y is at most n u kappa and that of a product of two y's 2 n u kappa; the n-term sums add n u:
             trace     relative  <= 4 n kappa u
             det_add   relative  <= 4 c n kappa u (1 + tr G): every entry of I + G moves by at most 4 n kappa u tr G (|G_kl| <=
                                 tr G), the c pivots of a positive definite matrix with eigenvalues >= 1 move by that much
                                 relative, and the elimination itself adds c u per pivot
             det_rm    absolute  <= 4 c^2 n kappa u on members of an exact design (eigenvalues of I - G in [0, 1]: no cofactor
                                 exceeds 1, c^2 entries each moved by at most 4 n kappa u tr G <= 4 n kappa u c).
"""
import functools
import json
import os

import mpmath
import numpy as np

import kinematics_common as kc
from figaroh_plus_amd.calibration import calibration_tools as ct
from figaroh_plus_amd.calibration import optimal_design as od

mpmath.mp.dps = 50
mpf = mpmath.mpf
U = 2.0 ** -53
SENTINEL = -6.02214076e23
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

MASKS = {3: (1, 1, 1, 0, 0, 0), 6: (1, 1, 1, 1, 1, 1)}
# (name, N, c, n): small enough for the exact restatement; "graded" scales column j by 10^(-6 j / (n - 1))
SMALL = (("one", 5, 1, 1), ("plain", 9, 3, 7), ("graded", 12, 6, 9), ("graded", 20, 2, 8), ("graded", 11, 4, 17))
EXACT_CANDIDATES = 24  # candidates of the fixture pool whose scores are restated exactly (evenly spread over the pool)


# ------------------------------------------------------------------------------------------------------------ problems
@functools.lru_cache(maxsize=None)
def fixture_configurations():
    """(model, q): the 500 postures of tests/golden/tiago_calibration_pool_500.json as configurations of the TIAGo model of
    the kinematics case "tiago_head_arm7" (head_2_joint -> a tool frame on arm_7_joint)."""
    case = kc.get_case("tiago_head_arm7")
    m = case.model
    with open(os.path.join(GOLD, "tiago_calibration_pool_500.json")) as f:
        d = json.load(f)
    cfg = np.array(d["calibration_joint_configurations"], dtype=np.float64)
    q = np.zeros((cfg.shape[0], m.nq))
    for j, name in enumerate(d["calibration_joint_names"]):
        q[:, m.joints[m.getJointId(name)].idx_q] = cfg[:, j]
    return case, q


@functools.lru_cache(maxsize=None)
def fixture_pool(c):
    """The base kinematic regressor of the fixture pool (full_params), component-major, from the float64 mirror: columns
    with squared norm >= 1e-6, then the columns whose diagonal entry in np.linalg.qr exceeds 1e-8 -- 34 of them."""
    case, q = fixture_configurations()
    R, _ = ct.kinematic_regressor_batch(case.model, q, case.end_joint, case.end_placement, case.start_joint,
                                        case.start_placement, case.support, want_R=True, want_J=False)
    W = kc.stack_measured(R, MASKS[c])
    keep = [j for j in range(W.shape[1]) if np.sum(W[:, j] ** 2) >= 1e-6]
    Rq = np.linalg.qr(W[:, keep], mode="r")
    base = [keep[k] for k in range(len(keep)) if abs(Rq[k, k]) > 1e-8]
    Rb = np.ascontiguousarray(W[:, base])
    Rb.setflags(write=False)
    return Rb


def random_problem(kind, N, c, n, seed=0):
    rng = np.random.default_rng(1000 * N + 10 * c + n + seed)
    R = rng.standard_normal((c * N, n))
    if kind == "graded" and n > 1:
        R = R * 10.0 ** (-6.0 * np.arange(n) / (n - 1))
    return R


def weights(N, kind, seed=0):
    """None, "random" (positive) or "zeros" (a third of the candidates at exactly 0.0, the last one never)."""
    if kind is None:
        return None
    rng = np.random.default_rng(77 + N + seed)
    w = rng.uniform(0.2, 1.5, N)
    if kind == "zeros":
        w[rng.permutation(N - 1)[:N // 3]] = 0.0
    return w


# ------------------------------------------------------------------------------------------------------ exact restatement
def _as_integers(A):
    """(object array of Python ints, K) with A = ints / 2^K exactly."""
    flat = [float(x).as_integer_ratio() for x in np.asarray(A, dtype=np.float64).ravel()]
    K = max(den.bit_length() - 1 for _, den in flat)
    out = np.empty(len(flat), dtype=object)
    for i, (num, den) in enumerate(flat):
        out[i] = num * ((1 << K) // den)
    return out.reshape(np.shape(A)), K


def exact_gram(R, N, c, w=None):
    """M = sum_i w_i sum_k r r^T without any rounding (integer arithmetic), as an object array of mpf."""
    Ri, KR = _as_integers(R)
    n = Ri.shape[1]
    if w is None:
        wi, KW = np.array([1] * N, dtype=object), 0
    else:
        wi, KW = _as_integers(w)
    acc = np.zeros((n, n), dtype=object)
    for k in range(c):
        blk = Ri[k * N:(k + 1) * N]
        acc = acc + (blk * wi[:, None]).T.dot(blk)
    scale = mpf(2) ** (2 * KR + KW)
    return np.array([[mpf(int(acc[a, b])) / scale for b in range(n)] for a in range(n)], dtype=object)


def gram_scale(R, N, c, w=None):
    A = np.abs(np.asarray(R, dtype=np.float64))
    S = np.zeros((A.shape[1],) * 2)
    for k in range(c):
        blk = A[k * N:(k + 1) * N]
        S += (blk if w is None else blk * w[:, None]).T @ blk
    return S


def gram_ratio(M, exact, R, N, c, w=None):
    """Largest |M_ab - exact| / ((c N + 2) u S_ab); entries with S_ab = 0 must be +0.0."""
    S = gram_scale(R, N, c, w)
    worst = 0.0
    for a in range(M.shape[0]):
        for b in range(M.shape[1]):
            if S[a, b] == 0.0:
                assert M[a, b] == 0.0
                continue
            worst = max(worst, float(abs(mpf(float(M[a, b])) - exact[a, b]) / ((c * N + 2) * U * S[a, b])))
    return worst


def gram_ratio_extended(M, R, N, c, w=None):
    """gram_ratio for shapes too large for integer arithmetic: the reference is formed in x87 extended precision
    (u_x = 2^-64), whose own error, at most (c N + 2) u_x S_ab, is taken OFF the bound -- the result is the largest
    |M_ab - reference| / ((c N + 2) (u - u_x) S_ab), and <= 1 implies the bound against the exact matrix."""
    assert np.finfo(np.longdouble).nmant >= 63, "no extended precision on this host"
    Rl = np.asarray(R, dtype=np.longdouble)
    ref = np.zeros((Rl.shape[1],) * 2, dtype=np.longdouble)
    for k in range(c):
        blk = Rl[k * N:(k + 1) * N]
        ref += (blk if w is None else blk * np.asarray(w, dtype=np.longdouble)[:, None]).T @ blk
    S = gram_scale(R, N, c, w)
    assert np.all(M[S == 0.0] == 0.0)
    err = np.abs(np.asarray(M, dtype=np.longdouble) - ref)[S > 0.0] / ((c * N + 2) * (U - 2.0 ** -64) * S[S > 0.0])
    return float(err.max()) if err.size else 0.0


def exact_scores(R, N, c, L, candidates):
    """{i: (tr G_i, det(I + G_i), det(I - G_i))} at 50 digits for the double factor L as given: y = L^-1 r, G = Y Y^T."""
    n = L.shape[0]
    Lm = [[mpf(float(L[a, b])) for b in range(a + 1)] for a in range(n)]
    out = {}
    for i in candidates:
        Y = []
        for k in range(c):
            r = [mpf(float(x)) for x in R[k * N + i]]
            y = []
            for a in range(n):
                s = r[a]
                for b in range(a):
                    s -= Lm[a][b] * y[b]
                y.append(s / Lm[a][a])
            Y.append(y)
        G = mpmath.matrix(c, c)
        for k in range(c):
            for l in range(c):
                G[k, l] = mpmath.fsum(Y[k][a] * Y[l][a] for a in range(n))
        eye = mpmath.eye(c)
        out[i] = (sum(G[k, k] for k in range(c)), mpmath.det(eye + G), mpmath.det(eye - G))
    return out


def score_ratios(got, exact, c, n, kappa):
    """Largest ratios of the three scores to their bounds over the exactly restated candidates."""
    t, add, rm = got
    worst = [0.0, 0.0, 0.0]
    for i, (te, ae, re) in exact.items():
        worst[0] = max(worst[0], float(abs(mpf(float(t[i])) - te) / (te * 4 * n * kappa * U)))
        worst[1] = max(worst[1], float(abs(mpf(float(add[i])) - ae) / (ae * 4 * c * n * kappa * U * (1 + te))))
        worst[2] = max(worst[2], float(abs(mpf(float(rm[i])) - re) / (4 * c * c * n * kappa * U)))
    return worst


@functools.lru_cache(maxsize=None)
def problem(name):
    """(R, N, c, n) of "fixture3", "fixture6" or "small<k>" (read-only arrays, computed once)."""
    if name.startswith("fixture"):
        c = int(name[-1])
        R = fixture_pool(c)
        return R, R.shape[0] // c, c, R.shape[1]
    kind, N, c, n = SMALL[int(name[5:])]
    R = random_problem(kind, N, c, n)
    R.setflags(write=False)
    return R, N, c, n


PROBLEMS = ("fixture3", "fixture6") + tuple("small%d" % k for k in range(len(SMALL)))


def exact_candidates(name):
    _, N, _, _ = problem(name)
    return list(range(N)) if N <= EXACT_CANDIDATES else [int(x) for x in np.linspace(0, N - 1, EXACT_CANDIDATES)]


@functools.lru_cache(maxsize=None)
def whole_design(name):
    """(M, L, kappa, exact scores) of the design that holds every candidate once: each candidate is a member."""
    R, N, c, n = problem(name)
    M = od.gram_mirror(R, N, c)
    L = np.linalg.cholesky(M)
    return M, L, float(np.linalg.cond(L)), exact_scores(R, N, c, L, exact_candidates(name))


# ------------------------------------------------------------------------------------------- the mirrors, with plants
GRAM_PLANTS = ("last_row_dropped", "neighbour_weight", "last_block_unweighted")
SCORE_PLANTS = ("L_transposed", "sign_swapped")


def planted_gram(R, N, c, w, plant):
    """optimal_design.gram_mirror with one error planted."""
    R = np.array(R, dtype=np.float64)
    if plant == "last_row_dropped":
        R[-1] = 0.0
        return od.gram_mirror(R, N, c, w)
    if plant == "neighbour_weight":
        return od.gram_mirror(R, N, c, np.roll(w, 1))
    assert plant == "last_block_unweighted"
    M = od.gram_mirror(R[:(c - 1) * N], N, c - 1, w) if c > 1 else np.zeros((R.shape[1],) * 2)
    return M + od.gram_mirror(R[(c - 1) * N:], N, 1, None)


def planted_scores(R, N, c, L, plant):
    """optimal_design.scores_mirror with one error planted."""
    if plant == "L_transposed":
        return od.scores_mirror(R, N, c, np.ascontiguousarray(L.T))
    assert plant == "sign_swapped"
    t, add, rm = od.scores_mirror(R, N, c, L)
    return t, rm, add


# ------------------------------------------------------------------------------------------------------ Detmax, restated
def detmax_pool(N=40, c=3, n=8, seed=4):
    return random_problem("plain", N, c, n, seed)


def brute_force_detmax(X, nd, initial_set):
    """The reference loop (optimal_config.py:82-126) on explicit X_i sums with numpy.linalg.det(...) ** (1 / n); returns
    (criteria, the set after every step, the smallest relative gap between the best and the second-best candidate of any
    add or remove scan)."""
    n = X[0].shape[0]

    def crit(idx):
        return float(np.linalg.det(sum(X[i] for i in idx)) ** (1.0 / n))

    pool_idx = tuple(range(len(X)))
    cur_set = list(initial_set)
    updated_pool = list(pool_idx)
    opt_k = updated_pool[0]
    opt_critD = crit(cur_set)
    rm_j = cur_set[0]
    out, sets, gap = [], [], np.inf
    while opt_k != rm_j:
        vals = []
        for k in updated_pool:
            cur_set.append(k)
            cur_critD = crit(cur_set)
            vals.append(cur_critD)
            if opt_critD < cur_critD:
                opt_critD = cur_critD
                opt_k = k
            cur_set.remove(k)
        top = sorted(vals)[-2:]
        gap = min(gap, (top[1] - top[0]) / top[1])
        cur_set.append(opt_k)
        opt_critD = crit(cur_set)
        delta_critD = opt_critD
        rm_j = cur_set[0]
        vals = []
        for j in cur_set:
            rm_set = cur_set.copy()
            rm_set.remove(j)
            cur_delta_critD = opt_critD - crit(rm_set)
            vals.append(cur_delta_critD)
            if cur_delta_critD < delta_critD:
                delta_critD = cur_delta_critD
                rm_j = j
        low = sorted(vals)[:2]
        gap = min(gap, (low[1] - low[0]) / opt_critD)
        cur_set.remove(rm_j)
        opt_critD = crit(cur_set)
        out.append(opt_critD)
        sets.append(list(cur_set))
    return out, sets, gap
