"""CPU suite: the native host tail (figh_chain_host_tail) against the Python tail it replaces --
``IdentificationPipeline._finish`` (n <= 80 branch), ``_host.null_rule_bounds`` and ``_host.null_rule_certified`` -- on inputs
built on the CPU: ``np.linalg.qr`` of small rank-deficient matrices laid out as figh_tsqr_selected lays its output out
(include/figh.h).  No device is needed: the entry is host only.

Tolerances.  Index sets, the verdict and the status are compared for equality.  ``beta`` is compared after rounding and must
be EQUAL: the dependent columns are built with coefficients of three decimals, so no unrounded reference entry lies within
1e-9 of a rounding boundary (checked here per case: the count of such entries must be zero; entries that differ elsewhere
fail the test, and more than 1 % of differing entries would fail it in any case).  ``phi_ls``, ``absdiagR`` and the bounds
agree to 1e-12 relative to the largest entry, plus -- for ``phi_ls`` and ``A_dep`` only -- the term the Python route carries
by construction and the native tail by design does not: LAPACK's dtrtri leaves the rounding residues BELOW the diagonal of
R1 in its output, and ``R1_inv @ R2`` multiplies them in; the test bounds that term by ``|L| |rhs|`` of the residues L it
planted itself."""
import os

import numpy as np
import pytest

from figaroh_plus_amd import _host, _lib
from figaroh_plus_amd.pipeline import IdentificationPipeline
from figaroh_plus_amd.tools import qrdecomposition as qrd

TOL = qrd.TOL_QR
ROWS = 240


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()


def make_rows(n, dep, with_tau, seed, rows=ROWS, residues=True):
    """((nc + 1) x nc rows_k, residues L (r x r, strictly lower), base, rest) of W = [independent columns | dependent columns
    = combinations, coefficients of three decimals, of the last base columns in front of them] (+ tau = W phi + noise)."""
    rng = np.random.default_rng(seed)
    dep = sorted(dep)
    base = [k for k in range(n) if k not in dep]
    W = np.zeros((rows, n))
    for k in range(n):
        front = [b for b in base if b < k][-3:]  # (at most three: the certificate's A_dep is the sum of the coefficients)
        if k in dep and front:
            W[:, k] = W[:, front] @ np.round(rng.uniform(-2.0, 2.0, len(front)), 3)
        else:
            assert k not in dep, "a dependent column needs a base column in front of it"
            W[:, k] = rng.standard_normal(rows)
    nc = n + (1 if with_tau else 0)
    M = W
    if with_tau:
        tau = W[:, base] @ rng.uniform(-3.0, 3.0, len(base)) + 0.05 * rng.standard_normal(rows)
        M = np.c_[W, tau]
    plain = np.linalg.qr(M, mode="r")
    perm = base + dep + ([n] if with_tau else [])
    Rr = np.linalg.qr(M[:, perm], mode="r")
    r = len(base)
    out = np.zeros((nc + 1, nc))
    for a, k in enumerate(base):
        out[k, perm] = Rr[a]
    if with_tau:
        out[n, n] = np.linalg.norm(Rr[r:, nc - 1])
    out[nc, :] = np.diag(plain)
    L = np.zeros((r, r))
    if residues and r > 1:
        L = np.tril(rng.standard_normal((r, r)), -1) * 1e-16 * np.abs(Rr[:r, :r]).max()
        for a in range(r):
            for b in range(a):
                out[base[a], base[b]] = L[a, b]
    return out, L, base, dep


def pipes(null_pivots=True):
    names = {"p%d" % i: 0.0 for i in range(80)}
    both = [IdentificationPipeline(None, None, params_std=names, native_tail=nt, null_pivots=null_pivots) for nt in (False, True)]
    for p in both:
        p.N = 10 ** 9  # (one separately launched piece whatever total_rows: IdentificationPipeline._level0_pieces)
    return both


def run_both(rows_k, n, with_tau, total_rows=ROWS, strings=True, null_pivots=True):
    nc = n + (1 if with_tau else 0)
    params_r = ["p%d" % i for i in range(n)]
    outs = []
    for p in pipes(null_pivots):
        outs.append(p._finish(rows_k.copy(), n, nc, list(params_r), [], np.zeros(n), with_tau, total_rows, strings))
    return outs


def reference_unrounded(rows_k, n, with_tau, base, rest):
    """(R1^-1 R2, R1^-1 z) from the upper triangle, for the rounding-boundary count."""
    Rb = rows_k[base]
    R1 = np.triu(Rb[:, base])
    X = np.linalg.solve(R1, np.c_[Rb[:, rest], Rb[:, n] if with_tau else np.zeros(len(base))]) if len(base) else np.zeros((0, len(rest) + 1))
    return X[:, :len(rest)], X[:, -1]


def near_boundary(x):
    """entries of x within 1e-9 of a point where rounding to six decimals changes (k + 1/2) 1e-6"""
    f = np.abs(x) * 1e6
    return int(np.count_nonzero(np.abs(f - np.floor(f) - 0.5) < 1e-3))


def compare(rows_k, L, n, with_tau, total_rows=ROWS, expect_certified=None):
    py, nat = run_both(rows_k, n, with_tau, total_rows)
    assert nat["idx_base"] == py["idx_base"] and nat["idx_e"] == py["idx_e"] and nat["params_r"] == py["params_r"]
    assert nat["null_rule_certified"] == py["null_rule_certified"]
    if expect_certified is not None:
        assert py["null_rule_certified"] is expect_certified
    assert nat["params_base"] == py["params_base"]
    base = py["idx_base"]
    rest = [k for k in range(n) if k not in base]
    unrounded, _ = reference_unrounded(rows_k, n, with_tau, base, rest)
    assert near_boundary(unrounded) == 0, "the reference itself has entries on a rounding boundary: choose another seed"
    assert nat["beta"].shape == py["beta"].shape
    differ = int(np.count_nonzero(nat["beta"] != py["beta"]))
    assert differ == 0 and differ <= 0.01 * max(1, py["beta"].size), "%d entries of beta differ" % differ
    np.testing.assert_array_equal(nat["absdiagR"], py["absdiagR"])  # (|x| is exact: no tolerance needed)
    if with_tau:
        Rb = rows_k[base]
        z = Rb[:, n]
        Xabs = np.abs(np.linalg.inv(np.triu(Rb[:, base]))) if base else np.zeros((0, 0))
        residue_term = (Xabs @ (np.abs(L) @ (Xabs @ np.abs(z)))).max(initial=0.0)
        bound = 1e-12 * np.abs(py["phi_ls"]).max(initial=0.0) + 2.0 * residue_term
        assert np.abs(nat["phi_ls"] - py["phi_ls"]).max(initial=0.0) <= bound
        np.testing.assert_array_equal(nat["phi_b"], np.round(nat["phi_ls"], 6))
        if near_boundary(py["phi_ls"]) == 0:
            np.testing.assert_array_equal(nat["phi_b"], py["phi_b"])
        assert nat["residual_norm"] == py["residual_norm"]
    return py, nat


CASES = {
    "n1_no_tau": (1, [], False, 11),
    "n3_tau": (3, [1], True, 12),
    "no_dependent_column": (5, [], True, 13),
    "one_base_rest_dependent": (4, [1, 2, 3], True, 14),
    "ur10_shape": (49, [6, 9, 13, 16, 20, 23, 27, 30, 34, 37, 41, 44, 47], True, 15),
    "n6_no_tau": (6, [2, 5], False, 16),
}


@pytest.mark.parametrize("name", list(CASES))
def test_native_tail_matches_python(name):
    n, dep, with_tau, seed = CASES[name]
    rows_k, L, base, rest = make_rows(n, dep, with_tau, seed)
    py, nat = compare(rows_k, L, n, with_tau, expect_certified=True)
    assert py["idx_base"] == base and len(py["idx_base"]) == n - len(dep)


def test_bounds_match_null_rule_bounds():
    n, dep, with_tau, seed = CASES["ur10_shape"]
    rows_k, L, base, rest = make_rows(n, dep, with_tau, seed)
    tail = _lib.HostTail(n, with_tau)
    s = tail.s
    s.tol_qr, s.total_rows, s.pieces, s.null_rule = TOL, ROWS, 1, 1
    _lib.chain_host_tail(tail, rows_k)
    assert s.bounds_recomputed == 1 and s.status == _lib.TAIL_OK and s.n_base == len(base)
    A_base, A_dep, xnorm = tail.bounds_tuple()
    Rb = rows_k[base]
    R1, R2 = np.triu(Rb[:, base]), Rb[:, rest]
    ref = _host.null_rule_bounds(R1, R2)
    # (null_rule_bounds reads the upper triangle only -- it is handed np.triu(R1) by _finish -- so the residues play no part)
    for got, want in ((A_base, ref[0]), (A_dep, ref[1]), (np.array([xnorm]), np.array([ref[2]]))):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # handed back with the same base columns, the bounds are used as they are: poison them and see the poison survive
    tail.keep_bounds(tail)
    tail.bounds[0] = 123.0
    _lib.chain_host_tail(tail, rows_k)
    assert s.bounds_recomputed == 0 and tail.bounds[0] == 123.0
    # ... and recomputed for another base set
    tail.cached_base[0] += 1
    _lib.chain_host_tail(tail, rows_k)
    assert s.bounds_recomputed == 1 and abs(tail.bounds[0] - ref[0][0]) <= 1e-12 * np.abs(ref[0]).max()


def test_zero_and_nan_pivot_are_not_base():
    n, dep, with_tau, seed = 6, [2, 4], True, 21
    rows_k, L, base, rest = make_rows(n, dep, with_tau, seed)
    rows_k[n + 1, 2] = 0.0
    py, nat = compare(rows_k, L, n, with_tau, expect_certified=True)
    assert py["idx_base"] == base
    rows_k[n + 1, 4] = np.nan
    py, nat = run_both(rows_k, n, with_tau)
    assert nat["idx_base"] == py["idx_base"] == base
    assert nat["null_rule_certified"] is False and py["null_rule_certified"] is False  # (a pivot that is not finite)
    assert np.isnan(nat["absdiagR"][4]) and nat["absdiagR"][2] == 0.0
    np.testing.assert_array_equal(nat["beta"], py["beta"])


def test_singular_r1_raises_in_both():
    n, dep, with_tau, seed = 5, [3], True, 22
    rows_k, L, base, rest = make_rows(n, dep, with_tau, seed)
    rows_k[1, 1] = 0.0
    for p in pipes():
        with pytest.raises(np.linalg.LinAlgError):
            p._finish(rows_k.copy(), n, n + 1, ["p%d" % i for i in range(n)], [], np.zeros(n), True, ROWS, True)
    tail = _lib.HostTail(n, with_tau)
    tail.s.tol_qr, tail.s.total_rows, tail.s.pieces, tail.s.null_rule = TOL, ROWS, 1, 1
    _lib.chain_host_tail(tail, rows_k)
    assert tail.s.status == _lib.TAIL_SINGULAR and tail.s.certified == 0 and tail.bounds_tuple() is None


@pytest.mark.parametrize("above", [True, False])
def test_dependent_pivot_around_an_eighth_of_the_tolerance(above):
    n, dep, with_tau, seed = 6, [2, 4], True, 23
    rows_k, L, base, rest = make_rows(n, dep, with_tau, seed)
    rows_k[n + 1, 4] = (TOL / 8.0) * (1.0 + (1e-9 if above else -1e-9))
    # (below tol_qr / 8 the margin 2 (1 + A_dep) tol_qr / 64 must still hold: A_dep <= 6 here, 7/32 < 7/8)
    compare(rows_k, L, n, with_tau, expect_certified=not above)


@pytest.mark.parametrize("inside", [True, False])
def test_base_pivot_around_the_sqrt_t_margin(inside):
    n, dep, with_tau, seed = 6, [2, 4], True, 24
    rows_k, L, base, rest = make_rows(n, dep, with_tau, seed)
    total_rows = 4_000_000
    Rb = rows_k[base]
    A_base = _host.null_rule_bounds(np.triu(Rb[:, base]), Rb[:, rest])[0]
    k = 3  # position of base column 5 among the base columns
    margin = (1.0 + A_base[k]) * (2.0 * TOL / _host.NULL_RULE_FOLD) * np.sqrt(_host.null_rule_triangles(total_rows, 1))
    rows_k[n + 1, base[k]] = TOL + margin * (1.0 - 1e-6 if inside else 1.0 + 1e-6)
    py, nat = compare(rows_k, L, n, with_tau, total_rows=total_rows, expect_certified=not inside)
    assert py["idx_base"] == base  # (above tol_qr either way: the column stays base, only the verdict changes)
    # the per-triangle margin alone would have let the pivot inside the sqrt(T) margin through
    assert margin > 100.0 * (1.0 + A_base[k]) * (2.0 * TOL / _host.NULL_RULE_FOLD)


def test_without_the_rule_no_verdict():
    n, dep, with_tau, seed = CASES["n3_tau"]
    rows_k, L, base, rest = make_rows(n, dep, with_tau, seed)
    py, nat = run_both(rows_k, n, with_tau, null_pivots=False)
    assert "null_rule_certified" not in py and "null_rule_certified" not in nat
    np.testing.assert_array_equal(nat["beta"], py["beta"])


def test_string_memo_hit_and_misses():
    n, dep, with_tau, seed = 6, [2, 4], True, 25
    rows_k, L, base, rest = make_rows(n, dep, with_tau, seed)
    p = pipes()[1]
    args = (n, n + 1, ["p%d" % i for i in range(n)], [], np.zeros(n), with_tau, ROWS, True)
    first = p._finish(rows_k.copy(), *args)
    assert p.strings_memo_hits == 0
    again = p._finish(rows_k.copy(), *args)
    assert p.strings_memo_hits == 1 and again["params_base"] == first["params_base"]
    again["params_base"][0] = "caller's copy"  # (the caller owns what it gets)
    assert p._finish(rows_k.copy(), *args)["params_base"] == first["params_base"] and p.strings_memo_hits == 2
    # fresh samples, same rounded coefficients: a perturbation far below 1e-6 of beta still hits
    moved = rows_k.copy()
    moved[base[0], rest[0]] *= 1.0 + 1e-13
    assert p._finish(moved, *args)["params_base"] == first["params_base"] and p.strings_memo_hits == 3
    # ... and so does the sign of a coefficient that rounds to zero (-0.0 / 0.0 follow R's rounding from run to run)
    moved = rows_k.copy()
    moved[base[-1], rest[0]] = 1e-12  # the last base row: beta[-1, 0] = 1e-12 / R1[-1, -1], +-0 after rounding
    zero = p._finish(moved.copy(), *args)
    hits = p.strings_memo_hits
    moved[base[-1], rest[0]] = -1e-12
    signed = p._finish(moved.copy(), *args)
    assert zero["beta"][-1, 0] == 0.0 and signed["beta"][-1, 0] == 0.0
    assert np.signbit(signed["beta"][-1, 0]) != np.signbit(zero["beta"][-1, 0])
    assert p.strings_memo_hits == hits + 1 and signed["params_base"] == zero["params_base"]
    p._finish(rows_k.copy(), *args)
    # a changed coefficient misses
    hits3 = p.strings_memo_hits
    moved = rows_k.copy()
    moved[base[0], rest[0]] += 1e-3 * moved[base[0], base[0]]
    changed = p._finish(moved, *args)
    assert p.strings_memo_hits == hits3 and changed["params_base"] != first["params_base"]
    assert changed["params_base"] == qrd._expressions(["p%d" % i for i in base], ["p%d" % i for i in rest], changed["beta"])
    # a changed index set misses: column 4 becomes base by its pivot (its row of the regrouped factorisation is zero, so
    # R1 would be singular -- give it a row)
    p._finish(rows_k.copy(), *args)
    hits = p.strings_memo_hits
    moved = rows_k.copy()
    moved[n + 1, 4] = 1.0
    moved[4, 4] = 1.0
    other = p._finish(moved, *args)
    assert p.strings_memo_hits == hits and other["idx_base"] == [0, 1, 3, 4, 5]
    assert len(other["params_base"]) == 5
