"""CPU suite of the posture selection (figaroh_plus_amd/calibration/optimal_design.py): the NumPy mirrors of the two passes
against an exact restatement with bounds that are derived in tests/design_common.py, five planted errors, the
multiplicative solve against the equivalence theorem and an independent scipy maximisation, Detmax against a brute-force
restatement of the reference loop, the two reference helpers against their loops, and the ValueError cases."""
import numpy as np
import pytest

import design_common as dc
from figaroh_plus_amd.calibration import optimal_design as od


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    """Every test here runs the mirrors, whatever the machine has."""
    monkeypatch.setattr(od._lib, "device_count", lambda: 0)


# ------------------------------------------------------------------------------------------------------------ mirrors
@pytest.mark.parametrize("wkind", [None, "random", "zeros"])
@pytest.mark.parametrize("name", dc.PROBLEMS)
def test_gram_mirror_against_exact(name, wkind, record_property):
    """|M_ab - exact| <= (c N + 2) u S_ab, exact symmetry, and exact zeros from zero weights."""
    R, N, c, n = dc.problem(name)
    w = dc.weights(N, wkind)
    M = od.gram_mirror(R, N, c, w)
    ratio = dc.gram_ratio(M, dc.exact_gram(R, N, c, w), R, N, c, w)
    record_property("gram_ratio", ratio)
    print("gram ratio %s %s: %.4f" % (name, wkind, ratio))
    assert np.array_equal(M, M.T)
    assert ratio <= 1.0
    # the extended-precision form of the check, which the GPU suite uses at larger shapes, is the stricter one
    assert ratio * (1 - 2.0 ** -11) - 2.0 ** -11 <= dc.gram_ratio_extended(M, R, N, c, w) <= (ratio + 2.0 ** -11) / (1 - 2.0 ** -11)
    if wkind == "zeros":  # the candidates with weight 0 contribute nothing: the same bits as without them
        keep = np.flatnonzero(w != 0.0)
        rows = np.concatenate([k * N + keep for k in range(c)])
        assert np.array_equal(M, od.gram_mirror(R[rows], len(keep), c, w[keep]))


@pytest.mark.parametrize("name", dc.PROBLEMS)
def test_scores_mirror_against_exact(name, record_property):
    """Trace, det(I + G) and det(I - G) of the design that holds every candidate, against 50 digits, with the derived
    bounds (kappa = cond_2(L) computed here)."""
    R, N, c, n = dc.problem(name)
    M, L, kappa, exact = dc.whole_design(name)
    ratios = dc.score_ratios(od.scores_mirror(R, N, c, L), exact, c, n, kappa)
    record_property("score_ratios", ratios)
    print("score ratios %s (kappa %.3g): trace %.4f det_add %.4f det_rm %.4f" % ((name, kappa) + tuple(ratios)))
    assert max(ratios) <= 1.0


@pytest.mark.parametrize("plant", dc.GRAM_PLANTS)
@pytest.mark.parametrize("name", dc.PROBLEMS)
def test_planted_gram_errors_are_caught(name, plant):
    R, N, c, n = dc.problem(name)
    w = dc.weights(N, "random")
    M = dc.planted_gram(R, N, c, w, plant)
    assert dc.gram_ratio(M, dc.exact_gram(R, N, c, w), R, N, c, w) > 1.0


# (L^T is L at n = 1: nothing would be planted in "small0")
@pytest.mark.parametrize("name,plant", [(name, plant) for name in dc.PROBLEMS for plant in dc.SCORE_PLANTS
                                        if not (plant == "L_transposed" and name == "small0")])
def test_planted_score_errors_are_caught(name, plant):
    R, N, c, n = dc.problem(name)
    M, L, kappa, exact = dc.whole_design(name)
    ratios = dc.score_ratios(dc.planted_scores(R, N, c, L, plant), exact, c, n, kappa)
    if plant == "sign_swapped":
        assert ratios[1] > 1.0 and ratios[2] > 1.0
    else:
        assert min(ratios) > 1.0


def test_det_rm_is_zero_off_the_design():
    """A candidate that is no member of the design can have M - X_i indefinite: det_rm is +0.0 there, and positive for
    every member of a design with a spare posture."""
    R, N, c, n = dc.problem("small1")
    pool = od.CandidatePool(R, N, c)
    design = [0, 1, 2, 3]
    d, add, rm = pool.scores(pool.subset_information_matrix(design))
    assert np.all(rm[design] > 0.0) and np.all(rm[design] < 1.0)
    off = [i for i in range(N) if i not in design]
    assert np.any(rm[off] == 0.0) and not np.any(np.signbit(rm)) and np.all(add >= 1.0)


# ------------------------------------------------------------------------------------------------------------- solvers
@pytest.mark.parametrize("c", [3, 6])
def test_multiplicative_design_is_optimal(c, capsys):
    """On the fixture pool the solve reaches max d <= n (1 + 1e-3) with sum w = 1 to rounding; on a 30-candidate sub-pool
    det(M(w))^(1/n) is within the certified efficiency bound of an independent scipy maximisation of log det over the
    simplex."""
    from scipy.optimize import minimize

    R = dc.fixture_pool(c)
    N, n = R.shape[0] // c, R.shape[1]
    pool = od.CandidatePool(R, N, c)
    solver = od.SOCP(pool, {"NbSample": N})
    w_list, w_dict_sort = solver.solve(tol=1e-3)
    w = np.array(w_list)
    print("c = %d: %d iterations, %d weights above 1e-5, cond M %.3g" % (c, solver.iterations, int(np.sum(w > 1e-5)),
                                                                        np.linalg.cond(pool.information_matrix(w))))
    assert solver.max_variance <= n * (1.0 + 1e-3) and solver.efficiency_bound >= 1.0 / (1.0 + 1e-3)
    # (sum_i w_i d_i = tr(M^-1 M) = n exactly, so an update keeps the sum up to the error of d, 4 n kappa u relative, and
    # three roundings of its own)
    kappa = max(np.sqrt(np.linalg.cond(pool.information_matrix(v))) for v in (None, w))
    assert abs(w.sum() - 1.0) <= solver.iterations * (4 * n * kappa + 3) * dc.U and np.all(w >= 0.0)
    assert list(w_dict_sort.values()) == sorted(w_list, reverse=True) and len(w_dict_sort) == N
    d = pool.scores(pool.information_matrix(w))[0]
    assert float(d.max()) == solver.max_variance
    # sub-pool: 30 candidates, evenly spread
    sub = np.linspace(0, N - 1, 30).astype(int)
    Rs = np.concatenate([R[k * N + sub] for k in range(c)])
    spool = od.CandidatePool(Rs, 30, c)
    ssolver = od.SOCP(spool, {"NbSample": 30})
    ws = np.array(ssolver.solve(tol=1e-3, max_iter=200000)[0])
    X = np.stack(od.sub_info_matrix(od.rearrange_rb(Rs, {"calibration_index": c, "NbSample": 30}),
                                    {"calibration_index": c, "NbSample": 30})[0])

    def neg_logdet(v):
        sign, ld = np.linalg.slogdet(np.tensordot(v, X, axes=1))
        return np.inf if sign <= 0 else -ld

    def grad(v):
        return -np.einsum("ab,iba->i", np.linalg.inv(np.tensordot(v, X, axes=1)), X)

    res = minimize(neg_logdet, np.full(30, 1.0 / 30), jac=grad, method="SLSQP", bounds=[(0.0, 1.0)] * 30,
                   constraints=[{"type": "eq", "fun": lambda v: v.sum() - 1.0, "jac": lambda v: np.ones(30)}],
                   options={"maxiter": 2000, "ftol": 1e-14})
    ours, theirs = np.exp(-neg_logdet(ws) / n), np.exp(-res.fun / n)
    print("sub-pool: ours %.12g scipy %.12g bound %.6f" % (ours, theirs, ssolver.efficiency_bound))
    assert ours >= ssolver.efficiency_bound * theirs  # the certificate bounds the optimum itself, hence any feasible point
    assert theirs >= ours * (1.0 - 1e-3)  # and scipy did find the optimum to the same tolerance
    capsys.readouterr()


def test_socp_takes_the_reference_dictionary_and_raises_at_max_iter(capsys):
    R, N, c, n = dc.problem("small1")
    param = {"calibration_index": c, "NbSample": N}
    _, subX_dict = od.sub_info_matrix(od.rearrange_rb(R, param), param)
    a, b = od.SOCP(subX_dict, param), od.SOCP(od.CandidatePool(R, N, c), param)
    wa, wb = np.array(a.solve(tol=1e-4)[0]), np.array(b.solve(tol=1e-4)[0])
    assert a.iterations == b.iterations and np.allclose(wa, wb, rtol=0, atol=1e-12)
    with pytest.raises(RuntimeError):
        od.SOCP(subX_dict, param).solve(tol=1e-9, max_iter=3)
    with pytest.raises(ValueError):
        od.SOCP(subX_dict, {"NbSample": N + 1})
    capsys.readouterr()


def test_detmax_equals_brute_force():
    """N = 40, c = 3, n = 8, NbChosen = 4 (n / c = 2.7): the sets after every step and the criteria equal those of the
    reference loop restated with numpy.linalg.det on explicit X_i sums.  No scan of the brute force is decided by a tie:
    its best and second-best candidates differ by at least 1e-8 relative at every step."""
    R = dc.detmax_pool()
    N, c, n, nd = 40, 3, 8, 4
    param = {"calibration_index": c, "NbSample": N}
    X, subX_dict = od.sub_info_matrix(od.rearrange_rb(R, param), param)
    initial = [17, 3, 29, 8]
    crit, sets, gap = dc.brute_force_detmax(X, nd, initial)
    assert len(crit) >= 2 and gap >= 1e-8, (len(crit), gap)
    for pool in (od.CandidatePool(R, N, c), subX_dict):
        algo = od.Detmax(pool, nd)
        got = algo.main_algo(initial_set=initial)
        assert got is algo.opt_critD and len(got) == len(crit)
        # (criteria: a determinant through LAPACK's LU against one through the Cholesky factor, both at a few n u cond)
        assert np.allclose(got, crit, rtol=1e-10, atol=0)
        assert sorted(algo.opt_set) == sorted(sets[-1]) and algo.opt_set == sets[-1]
        assert all(b >= a * (1 - 1e-12) for a, b in zip(got, got[1:]))
    # the random start draws NbChosen distinct candidates
    algo = od.Detmax(od.CandidatePool(R, N, c), nd)
    algo.main_algo(rng=3)
    assert len(algo.opt_set) == nd and len(set(algo.opt_set)) == nd


# ------------------------------------------------------------------------------------------- helpers and refusals
def test_rearrange_and_sub_info_matrix_against_the_reference_loops():
    R, N, c, n = dc.problem("small2")
    param = {"calibration_index": c, "NbSample": N}
    want = np.empty_like(R)
    for i in range(c):
        for j in range(N):
            want[j * c + i, :] = R[i * N + j]
    got = od.rearrange_rb(R, param)
    assert np.array_equal(got, want)
    subX_list, subX_dict = od.sub_info_matrix(got, param)
    assert list(subX_dict.keys()) == list(range(N)) and len(subX_list) == N
    for it in range(N):
        sub_R = want[it * c:(it * c + c), :]
        scale = np.matmul(np.abs(sub_R).T, np.abs(sub_R))
        assert np.all(np.abs(subX_list[it] - np.matmul(sub_R.T, sub_R)) <= 2 * c * dc.U * scale)
        assert subX_dict[it] is subX_list[it]
    # the pool's information matrix is the sum of the X_i, and detroot_whole follows :257-264
    pool = od.CandidatePool(R, N, c)
    M = pool.information_matrix()
    assert np.allclose(M, sum(subX_list), rtol=1e-13, atol=0)
    assert np.isclose(od.detroot_whole(pool), np.linalg.det(np.matmul(want.T, want)) ** (1.0 / n) / np.sqrt(n), rtol=1e-10)
    assert np.allclose(pool.subset_information_matrix([1, 4, 4]), subX_list[1] + 2 * subX_list[4], rtol=1e-12, atol=1e-300)


def test_value_errors_and_selection():
    R, N, c, n = dc.problem("small1")
    with pytest.raises(ValueError, match="rows were deleted"):
        od.CandidatePool(R[:-1], N, c)
    with pytest.raises(ValueError, match="columns"):
        od.CandidatePool(np.zeros((c * N, od.MAX_COLS + 1)), N, c)
    with pytest.raises(ValueError):
        od.CandidatePool(np.zeros((7 * N, 4)), N, 7)
    pool = od.CandidatePool(R, N, c)
    with pytest.raises(ValueError):
        pool.information_matrix(np.ones(N + 1))
    with pytest.raises(ValueError):
        pool.subset_information_matrix([0, N])
    with pytest.raises(np.linalg.LinAlgError):
        pool.scores(pool.subset_information_matrix([0]))  # rank c < n
    w_dict_sort = {4: 0.5, 1: 0.3, 7: 0.2 - 2e-6, 2: 2e-6, 0: 0.0}
    assert od.select_configurations(w_dict_sort, min_chosen=3) == [4, 1, 7]
    with pytest.raises(AssertionError, match="Infeasible design"):
        od.select_configurations(w_dict_sort, min_chosen=4)
    assert od.minNbChosen({"calib_model": "full_params", "actJoint_idx": list(range(7)), "calibration_index": 3}) == 15
    assert od.minNbChosen({"calib_model": "joint_offset", "actJoint_idx": list(range(7)), "calibration_index": 3}) == 3
    with pytest.raises(AssertionError):
        od.minNbChosen({"calib_model": "other", "actJoint_idx": [], "calibration_index": 3})
    import figaroh_plus_amd.calibration as cal
    assert cal.SOCP is od.SOCP and cal.Detmax is od.Detmax and cal.CandidatePool is od.CandidatePool
