"""GPU suite: column-wise accuracy of the TSQR kernels on graded matrices, against references that are exact by construction.

The older QR checks of test_gpu_parity.py normalise by the largest entry of the whole problem, so a column 10^4 smaller
than the largest is checked only to 10^-8 of its own size.  The decisions of qrdecomposition.py:205-221 (|R_kk| > tol_qr)
and the null-pivot rule (tol_qr / 64 per level-0 triangle) are absolute thresholds, i.e. they read every column at its own
scale.  Here the inputs are integer matrices with power-of-two column scales (tests/qr_graded_common.py): their Gram matrix
is exact in float64 and its long-double Cholesky factor is the reference R, accurate column by column.  Three metrics,
each divided by the norms of the columns it reads:

* backward  max_ij |R^T R - G|_ij / (|a_i| |a_j|)        (Householder QR is backward stable column by column)
* forward   max_j |R[:, j] - R_ref[:, j]| / |a_j|      against c cond u, cond of the column-equilibrated matrix
* diagonal  max_k | |R_kk| - R_ref_kk | / |a_k|         what the base-parameter decision reads

Tolerances: ten times (or more) the largest value measured on an MI355X over the whole sweep; the measured values are
recorded as test properties (``--junitxml``).  The backward tolerance is far below the 1e-12 the suite uses norm-wise.
"""
import numpy as np
import pytest

import qr_graded_common as qg

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TOL_QR = 1e-8
NULL_TOL = TOL_QR / 64
# largest value measured over the whole sweep on an MI355X -> tolerance (>= 10x margin)
TOL_BACKWARD = qg.TOL_BACKWARD  # measured 5.2e-15 (rfactor 20011 x 511, wide profile; 7.7e-15 with dependent columns)
C_FORWARD = 200.0     # forward <= C_FORWARD cond u: measured 17.6 cond u (rfactor 20011 x 511, wide)
C_DIAG = 200.0        # diagonal <= C_DIAG cond u: measured 17.3 cond u (same case)

PROFILES = qg.PROFILES
NS = [1, 15, 16, 17, 49, 63, 64, 65, 79, 80, 81, 96, 97, 193, 272, 321, 336, 385, 400, 511]


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    qg.check_longdouble()
    return _lib


def _pow2(s):
    return np.ldexp(1.0, np.asarray(s, dtype=np.int64))


def _check(R, G, record_property, tag, forward=True, backward_tol=TOL_BACKWARD, R_ref=None, triangular=True):
    """Assert the three metrics (forward / diagonal only with a full-rank reference) and record them."""
    if triangular:
        assert np.array_equal(R, np.triu(R))
    b = qg.backward_err(R, G)
    record_property(tag + ":backward", "%.3e" % b)
    assert b <= backward_tol, "%s: backward %.3e > %.1e" % (tag, b, backward_tol)
    if not forward:
        return
    if R_ref is None:
        R_ref = qg.cholesky_ld(G)
    cond = qg.equilibrated_cond(R_ref)
    # the reference's own column-wise error, cond^2 * 2^-64, must stay a tenth of what the kernel is allowed
    assert cond * cond * 2.0 ** -64 <= 0.1 * cond * U, "input too ill-conditioned for the long-double reference"
    f, d = qg.forward_err(R, R_ref, G), qg.diag_err(R, R_ref, G)
    record_property(tag + ":forward_over_cond_u", "%.3e" % (f / (cond * U)))
    record_property(tag + ":diag_over_cond_u", "%.3e" % (d / (cond * U)))
    assert f <= C_FORWARD * cond * U, "%s: forward %.3e > %g cond u (cond %.3g)" % (tag, f, C_FORWARD, cond)
    assert d <= C_DIAG * cond * U, "%s: diagonal %.3e > %g cond u (cond %.3g)" % (tag, d, C_DIAG, cond)


def _graded(rng, rows, n, profile):
    lo, hi = PROFILES[profile]
    M = qg.int_matrix(rng, rows, n)
    s = qg.graded_scales(rng, n, lo, hi, qg.small_positions(n))
    return M, s


# ---------------------------------------------------------------------------------------------------- level 0 + merges
@pytest.mark.parametrize("profile", sorted(PROFILES))
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("rows", [64, 1000, 20011])
def test_rfactor_graded_columns(lib, rows, n, profile, record_property):
    """figh_tsqr on graded integer matrices: one wave, tsqr2 4 and 5 chunks, every geometry of the blocked kernel, with the
    smallest columns first, last and on the panel / chunk boundaries.  Backward for every shape, forward and diagonal
    against the exact Cholesky factor when rows >= 2n."""
    from figaroh_plus_amd.tools.qrdecomposition import rfactor
    rng = np.random.default_rng([n, rows, len(profile)])
    M, s = _graded(rng, rows, n, profile)
    R = rfactor(M * _pow2(s))
    _check(R, qg.exact_gram(M, s), record_property, "rfactor", forward=rows >= 2 * n)


@pytest.mark.parametrize("profile", sorted(PROFILES))
@pytest.mark.parametrize("n", [15, 64, 79, 96, 193, 336, 400])
@pytest.mark.parametrize("rows", [64, 1000, 20008])
def test_rfactor_graded_tau_gather_weights(lib, rows, n, profile, record_property):
    """The same with a graded tau column, the columns gathered out of a wider ld (unsorted col_idx) and power-of-two row
    block weights: the exact Gram of [W[:, idx] tau] with the block rows scaled."""
    from figaroh_plus_amd.tools.qrdecomposition import rfactor
    rng = np.random.default_rng([n, rows, len(profile), 7])
    ld = n + 7
    Mw, sw = _graded(rng, rows, ld, profile)
    idx = rng.permutation(ld)[:n].astype(np.int32)
    lo, hi = PROFILES[profile]
    mt, st = qg.int_matrix(rng, rows, 1)[:, 0], int(rng.integers(lo, hi + 1))
    nb = 8
    e = rng.integers(-1, 2, nb)
    R = rfactor(Mw * _pow2(sw), tau=mt * 2.0 ** st, col_idx=idx, block_weight=_pow2(e))
    M = np.c_[Mw[:, idx], mt]
    G = qg.exact_gram(M, np.r_[sw[idx], st], np.repeat(e, rows // nb))
    _check(R, G, record_property, "rfactor_tau_gather_weights", forward=rows >= 2 * (n + 1))


def test_rfactor_graded_48_row_form(lib, record_property):
    """72 columns (71 + tau) at 10^6 rows: level 0 runs as the 48-row form (tsqr2_kernel<5, 3, ...)."""
    from figaroh_plus_amd.tools.qrdecomposition import rfactor
    rng = np.random.default_rng(72)
    rows, n, ld = 1000000, 71, 80
    for profile in sorted(PROFILES):
        Mw, sw = _graded(rng, rows, ld, profile)
        idx = np.sort(rng.choice(ld, n, replace=False)).astype(np.int32)
        mt = qg.int_matrix(rng, rows, 1)[:, 0]
        R = rfactor(Mw * _pow2(sw), tau=mt * 0.5, col_idx=idx)
        G = qg.exact_gram(np.c_[Mw[:, idx], mt], np.r_[sw[idx], -1])
        _check(R, G, record_property, "rfactor_48_row_form")


_graded_triangles = qg.graded_triangles  # (importable without pytest: the call-sequence worker builds the same stacks)


MERGE_CASES = [(1, 5), (17, 40), (50, 2), (50, 16), (50, 300), (50, 2039), (64, 700), (65, 9), (80, 130), (49, 4500), (81, 2),
               (120, 7), (191, 33), (241, 5), (331, 16), (336, 3), (400, 2), (511, 3)]


@pytest.mark.parametrize("profile", sorted(PROFILES))
@pytest.mark.parametrize("nc,count", MERGE_CASES)
def test_merge_graded_columns(lib, nc, count, profile, record_property):
    """figh_tsqr_merge on graded integer triangle stacks: coop kernels, one-launch stream, the level-by-level tree (4500
    triangles) and the wide pair merges, against the exact Cholesky factor of the stacked rows."""
    rng = np.random.default_rng([nc, count, len(profile)])
    T, s = _graded_triangles(rng, count, nc, profile)
    A = (T * _pow2(s)).reshape(-1, nc)
    d_stack = lib.DeviceArray.from_host(A.reshape(-1))
    d_R = lib.DeviceArray((nc * nc,))
    lib.tsqr_merge(d_stack, count, nc, d_R)
    R = d_R.to_host().reshape(nc, nc)
    _check(R, qg.exact_gram(T.reshape(-1, nc), s), record_property, "merge")


def _make_dependent(rng, X, s, n, lo):
    """Every third column k < n an exact combination of earlier base columns (qr_graded_common.make_dependent, one class
    for all columns).  Returns (dependent, base) column lists."""
    return qg.make_dependent(rng, X, s, n, lo)


@pytest.mark.parametrize("profile", sorted(PROFILES))
@pytest.mark.parametrize("nc,count,with_tau", [(50, 1, True), (50, 8, True), (37, 200, False), (70, 33, True), (50, 2039, True),
                                               (120, 3, True), (200, 1, False), (331, 4, True)])
def test_merge_base_graded_exact_dependencies(lib, nc, count, with_tau, profile, record_property):
    """figh_tsqr_merge_base (rank-revealing merge + device permutation) on graded stacks with exact dependencies: the base
    set is the exact one, every true pivot at least 3x away from tol_qr; the regrouped base triangle against the exact
    Cholesky factor of the base columns; the regrouped rows against the exact Gram."""
    rng = np.random.default_rng([nc, count, len(profile), 11])
    n = nc - (1 if with_tau else 0)
    T, s = _graded_triangles(rng, count, nc, profile)
    dep, base = _make_dependent(rng, T, s, n, PROFILES[profile][0])
    Mi = T.reshape(-1, nc)
    G = qg.exact_gram(Mi, s)
    base_n = [k for k in base if k < n]
    R_ref = qg.cholesky_ld(G[np.ix_(base_n, base_n)])
    assert float(np.diag(R_ref).min()) >= 3 * TOL_QR  # the exact decision does not depend on rounding
    d_stack = lib.DeviceArray.from_host((T * _pow2(s)).reshape(-1))
    d_out = lib.DeviceArray(((nc + 1) * nc,))
    lib.tsqr_merge_base(d_stack, count, nc, n, TOL_QR, d_out)
    rows_k = d_out.to_host().reshape(nc + 1, nc)
    d = np.abs(rows_k[nc])
    assert np.flatnonzero(d[:n] > TOL_QR).tolist() == base_n
    assert d[dep].max(initial=0.0) <= TOL_QR / 3
    assert not rows_k[dep].any()
    R1 = np.triu(rows_k[base_n][:, base_n])
    _check(R1, G[np.ix_(base_n, base_n)], record_property, "merge_base_R1", R_ref=R_ref)
    keep = base_n + ([n] if with_tau else [])
    _check(rows_k[keep], G, record_property, "merge_base_rows", forward=False, triangular=False)


# ---------------------------------------------------------------------------------------------------- null-pivot rule
def _fold_term(G, rows):
    """Column-wise bound of what the rule may fold: (tol_qr / 64) sqrt(T) (|a_i| + |a_j|) / (|a_i| |a_j|), T bounded as in
    the guard (_host.null_rule_triangles)."""
    from figaroh_plus_amd._host import null_rule_triangles
    nrm = qg.col_norms(G)
    nrm = np.where(nrm > 0, nrm, 1.0)
    T = null_rule_triangles(rows)
    return NULL_TOL * np.sqrt(T) * (nrm[:, None] + nrm[None, :]) / np.outer(nrm, nrm)


@pytest.mark.parametrize("profile", sorted(PROFILES))
@pytest.mark.parametrize("n,rows", [(50, 4096), (64, 50011), (80, 4096), (96, 50011), (241, 4096), (331, 50011), (400, 4096)])
def test_null_pivot_rule_graded_column_bound(lib, n, rows, profile, record_property):
    """With the rule on, R is the exact factor of W + E, at most tol_qr / 64 folded per column per level-0 triangle:
    column by column, |R^T R - G|_ij <= backward tol |a_i| |a_j| + (tol_qr / 64) sqrt(T) (|a_i| + |a_j|).  Graded matrices
    with exact dependencies (every third column); the base set equals the exact one with the rule on and off."""
    from figaroh_plus_amd import _lib
    from figaroh_plus_amd.tools.qrdecomposition import rfactor
    rng = np.random.default_rng([n, rows, len(profile), 13])
    lo, hi = PROFILES[profile]
    M = qg.int_matrix(rng, rows, n)
    s = qg.graded_scales(rng, n, lo, hi, qg.small_positions(n))
    dep, base = _make_dependent(rng, M, s, n, lo)
    G = qg.exact_gram(M, s)
    assert float(np.diag(qg.cholesky_ld(G[np.ix_(base, base)])).min()) >= 3 * TOL_QR
    A = M * _pow2(s)
    nrm = np.where(qg.col_norms(G) > 0, qg.col_norms(G), 1.0)
    for tol in (0.0, NULL_TOL):
        with _lib.null_pivots(64 * tol):
            R = rfactor(A)
        assert np.flatnonzero(np.abs(np.diag(R)) > TOL_QR).tolist() == base
        Rl = np.asarray(R, dtype=np.longdouble)
        E = np.abs(Rl.T @ Rl - np.asarray(G, dtype=np.longdouble)) / np.outer(nrm, nrm).astype(np.longdouble)
        bound = TOL_BACKWARD + (_fold_term(G, rows) if tol else 0.0)
        record_property("null_rule_%g:backward_over_bound" % tol, "%.3e" % float((E / bound).max()))
        assert (E <= bound).all(), "rule %g: column-wise backward error above the bound" % tol


# ------------------------------------------------------------------------------------ adversarial family for the null rule
ADV_ROWS, ADV_N = 4000000, 50
ADV_DEP = [9, 27, 41, 47]  # 9, 27: combinations of large columns; 41 <- column 20, 47 <- column 33 (+ large ones)


def _adversarial(variant, seed=2024):
    """4e6 x 50: large random columns, two genuine base columns (20, 33) with exact pivots between 2e-8 and 1e-7 -- the
    distance of their residual (a random +-1 vector, independent of the other columns) from the columns in front of them,
    its length up to a relative 1e-5 -- and columns 41, 47 exact combinations of them (coefficients 0.3 .. 3) and of large
    earlier columns.  Every true pivot is at least 2x away from tol_qr.

    ``uniform``: the residual is spread evenly over the rows (per 64-row tile far below tol_qr / 64).  ``spread-T``: most of
    the pivot sits in the first 8192 rows; everywhere else the residual is just below tol_qr / 64 per level-0 triangle,
    assuming T triangles of interleaved tiles -- a column the rule folds in almost every triangle."""
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((ADV_ROWS, ADV_N))
    W *= rng.uniform(0.5, 5.0, ADV_N)
    W[:, 9] = W[:, [1, 4, 7]] @ np.array([0.5, -1.2, 2.0])
    W[:, 27] = W[:, [3, 12, 25]] @ np.array([1.5, 0.7, -0.4])
    pivots = {}
    for col, p, alpha, dcol, big in ((20, 3e-8, 2.5, 41, [2, 15]), (33, 4.5e-8, -3.0, 47, [5, 30])):
        src = [k for k in range(col) if k not in ADV_DEP]
        z = rng.choice([-1.0, 1.0], ADV_ROWS)
        if variant == "uniform":
            r = z * (p / np.sqrt(ADV_ROWS))
        else:
            T = int(variant.split("-")[1])
            small = 0.9 * NULL_TOL / np.sqrt(ADV_ROWS / T)
            r = z * small
            head = 8192
            rest = p * p - small * small * ADV_ROWS
            r[:head] = z[:head] * np.sqrt(rest / head + small * small)
        W[:, col] = W[:, src] @ rng.uniform(-1.0, 1.0, len(src)) + r
        pivots[col] = float(np.linalg.norm(r))
        W[:, dcol] = alpha * W[:, col] + W[:, big] @ rng.uniform(-2.0, 2.0, len(big))
    for p in pivots.values():
        assert 2 * TOL_QR <= p <= 1e-7
    base = [k for k in range(ADV_N) if k not in ADV_DEP]
    tau = W @ rng.uniform(-1.0, 1.0, ADV_N) + 0.01 * rng.standard_normal(ADV_ROWS)
    return W, tau, base


@pytest.mark.timeout(900)
@pytest.mark.parametrize("variant", ["uniform", "spread-1024", "spread-2048"])
def test_null_rule_adversarial_base_pivots(lib, variant):
    """The entries that use the null-pivot rule by default (get_baseIndex, get_baseParams, double_QR) on the adversarial
    family: idx_base equals the exact reference's.  A base column the rule folds in almost every triangle keeps its
    direction in the columns behind it; an exactly dependent column may then show a spurious pivot above tol_qr, which the
    guard has to catch (the factorisation is then repeated without the rule)."""
    from figaroh_plus_amd.device import GpuMatrix
    from figaroh_plus_amd.tools import qrdecomposition as qrd
    W, tau, base = _adversarial(variant)
    Wd = GpuMatrix.from_host(W)
    del W
    params = ["p%d" % k for k in range(ADV_N)]
    got = {
        "get_baseIndex": list(qrd.get_baseIndex(Wd, params)),
        "get_baseParams": list(qrd.get_baseParams(Wd, params)[2]),
        "double_QR": [params.index(p.split(" ")[0]) for p in qrd.double_QR(tau, Wd, params)[2]],
        "plain Householder": list(qrd.get_baseIndex(Wd, params, null_pivots=False)),
    }
    for entry, idx in got.items():
        assert idx == base, "%s (%s): idx_base %s, exact %s" % (entry, variant, idx, base)


# ---------------------------------------------------------------------------------------------------- kernel-built W
def _gram_ld(A):
    """Gram matrix of a float64 matrix in long double: its own column-wise error is at most rows * 2^-64 |a_i| |a_j|
    (rows <= 2e5 here: below 1.1e-14, a tenth of TOL_BACKWARD), where the float64 Gram's is about sqrt(rows) u."""
    Al = np.asarray(A, dtype=np.longdouble)
    return Al.T @ Al


def _check_against_W(R, A, record_property, tag):
    """Backward metric of a kernel-built W's triangle against the long-double Gram of that W, and the evidence that the
    float64 Gram would have been good enough as well: its column-wise error lies far below the tolerance."""
    assert A.shape[0] * 2.0 ** -64 <= 0.1 * TOL_BACKWARD
    G = _gram_ld(A)
    nrm = np.sqrt(np.diag(G).astype(np.float64))
    nrm = np.where(nrm > 0, nrm, 1.0)
    g64 = float((np.abs(np.asarray(A.T @ A, dtype=np.longdouble) - G) / np.outer(nrm, nrm)).max())
    record_property(tag + ":fp64_gram_error", "%.3e" % g64)
    assert g64 <= 0.1 * TOL_BACKWARD
    assert np.array_equal(R, np.triu(R))
    Rl = np.asarray(R, dtype=np.longdouble)
    b = float((np.abs(Rl.T @ Rl - G) / np.outer(nrm, nrm)).max())
    record_property(tag + ":backward", "%.3e" % b)
    record_property(tag + ":column_norm_spread", "%.3e" % (nrm.max() / nrm[nrm > 1.0e-300].min()))
    assert b <= TOL_BACKWARD, "%s: backward %.3e > %.1e" % (tag, b, TOL_BACKWARD)


def test_fused_chain_and_two_launch_columnwise(lib, record_property):
    """figh_regressor_tsqr_fused (K1 + level-0 TSQR in one launch, tol_qr < 0: the plain triangle) against the Gram of the
    W it wrote, read back; then the two-launch form (the regressor kernel, then figh_tsqr) on that same device W."""
    from conftest import Golden
    from figaroh_plus_amd.tools.regressor import _samples_to_device
    g = Golden("cfg2_ur10")
    N = 8192 + 17
    rng = np.random.default_rng(5)
    q, v, a = (rng.uniform(-6, 6, (N, 6)) for _ in range(3))
    tau = rng.standard_normal(6 * N)
    kept = np.array([c for c in range(84) if c not in set(int(x) for x in g["idx_e"])], dtype=np.int32)
    n, nc = len(kept), len(kept) + 1
    robot = g.robot()
    _, d_q, d_v, d_a = _samples_to_device(robot.model, q, v, a)
    d_W = lib.DeviceArray((6 * N * 84,), np.float64)
    d_cs = lib.DeviceArray((84,), np.float64)
    d_kept = lib.DeviceArray.from_host(kept)
    d_tau = lib.DeviceArray.from_host(tau)
    d_R = lib.DeviceArray((nc * nc,), np.float64)
    assert lib.regressor_tsqr_fused(robot.device_model(), 0, N, d_q, d_v, d_a, d_W, 84, d_cs, d_kept, n, d_tau, -1.0, d_R)
    W = d_W.to_host().reshape(6 * N, 84)
    A = np.c_[W[:, kept], tau]
    _check_against_W(np.triu(d_R.to_host().reshape(nc, nc)), A, record_property, "fused_chain")
    lib.tsqr(d_W, 6 * N, 84, d_kept, n, d_tau, None, d_R)
    _check_against_W(np.triu(d_R.to_host().reshape(nc, nc)), A, record_property, "two_launch")


@pytest.mark.parametrize("cfg", ["cfg1_tx40", "cfg2_ur10", "cfg3_tiago", "cfg4_talos", "cfg5_human"])
def test_tsqr_selected_columnwise(lib, cfg, record_property):
    """figh_tsqr_selected (elimination + TSQR on the device, tol_qr < 0: the plain triangle of the kept columns + tau) on
    the regressor the device built -- TIAGo's kept columns span 7e4 in norm -- against the Gram of that W, read back."""
    from conftest import Golden
    from figaroh_plus_amd.tools.regressor import build_regressor_device, regressor_flags
    g = Golden(cfg)
    robot = g.robot()
    q, v, a = g["q_big"], g["v_big"], g["a_big"]
    N = len(q)
    dq, dv, da = (lib.DeviceArray.from_host(np.ascontiguousarray(x).reshape(-1)) for x in (q, v, a))
    W, colsq = build_regressor_device(robot, dq, dv, da, N, g.param, coupling=g.coupling, colsq=True)
    ncols = W.cols
    mode, _, _ = regressor_flags(g.param, g.coupling)
    m = robot.model
    nblocks = m.nv if (mode == lib.MODE_JOINT_TORQUE and m.nv == m.njoints - 1 and N >= 64) else 0
    tau = g["tau"]
    d_tau = lib.DeviceArray.from_host(tau)
    d_sel = lib.DeviceArray((2 + 2 * ncols,), np.int32)
    kept = [i for i in range(ncols) if i not in set(g["idx_e"].tolist())]
    n = len(kept)
    d_R = lib.DeviceArray(((n + 1) * (n + 1),))
    lib.tsqr_selected(W.buf, W.rows, W.ld, colsq, ncols, 1e-6, 14, nblocks, n, d_tau, -1.0, d_sel, d_R)
    assert d_sel.to_host()[2:2 + n].tolist() == kept
    Wh = np.empty((W.rows, W.ld))
    lib.check(lib.load().figh_memcpy_d2h(Wh.ctypes.data, W.buf.ptr, Wh.nbytes))
    _check_against_W(np.triu(d_R.to_host().reshape(n + 1, n + 1)), np.c_[Wh[:, kept], tau], record_property,
                     "tsqr_selected")


@pytest.mark.parametrize("chunk", [0, 64])
@pytest.mark.parametrize("cfg", ["cfg1_tx40", "cfg2_ur10", "cfg3_tiago", "cfg4_talos", "cfg5_human"])
def test_streamed_regressor_tsqr_columnwise(lib, cfg, chunk, record_property):
    """figh_regressor_tsqr (W never stored; chunk > 0: the samples in chunks, one set of level-0 triangles each) against
    the Gram of the W the same regressor kernels write when W is materialised, read back."""
    from conftest import Golden
    from figaroh_plus_amd.tools.regressor import add_coupling_TX40, build_regressor_basic, regressor_flags
    g = Golden(cfg)
    q, v, a, tau = g["q_big"], g["v_big"], g["a_big"], g["tau"]
    N = len(q)
    robot = g.robot()
    W = build_regressor_basic(robot, q, v, a, dict(g.param))
    if g.coupling:  # TX40: the coupling columns, which the streamed kernel forms in the same pass
        m = robot.model
        W = add_coupling_TX40(W, m, robot.data, N, m.nq, m.nv, m.njoints, q, v, a)
    dm = robot.device_model()
    mode, flags, ft = regressor_flags(g.param, g.coupling)
    rps, ncols = dm.shape(mode, flags)
    assert W.shape == (rps * N, ncols)
    d_q, d_v, d_a = (lib.DeviceArray.from_host(np.ascontiguousarray(x).reshape(-1)) for x in (q, v, a))
    keep = [i for i in range(ncols) if i not in set(g["idx_e"].tolist())]
    n = len(keep)
    d_idx = lib.DeviceArray.from_host(np.asarray(keep, dtype=np.int32))
    d_R = lib.DeviceArray(((n + 1) * (n + 1),))
    lib.regressor_tsqr(dm, mode, flags, ft, N, d_q, d_v, d_a, d_idx, n, lib.DeviceArray.from_host(tau), None, d_R,
                       chunk_samples=chunk)
    _check_against_W(np.triu(d_R.to_host().reshape(n + 1, n + 1)), np.c_[W[:, keep], tau], record_property,
                     "streamed_chunk%d" % chunk)


# ---------------------------------------------------------------------------------------------------- the pipeline's guard
@pytest.mark.parametrize("chunk", [None, 5000])
def test_pipeline_guard_reads_the_rows_of_the_pass(lib, monkeypatch, chunk):
    """IdentificationPipeline certifies its passes with the row count of the whole factorisation (6N for UR10, all chunks)
    and the number of separately launched parts: the sqrt(T) margin of _host.null_rule_certified reads them.  The guard is
    observed through a wrapper; the pass is certified and does not fall back."""
    from conftest import Golden
    from figaroh_plus_amd import _host
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    g = Golden("cfg2_ur10")
    N = 20000
    rng = np.random.default_rng(31)
    q, v, a = (rng.uniform(-6, 6, (N, 6)) for _ in range(3))
    seen = []
    real = _host.null_rule_certified

    def spy(*args, **kw):
        seen.append((kw.get("rows"), kw.get("pieces")))
        return real(*args, **kw)

    monkeypatch.setattr(_host, "null_rule_certified", spy)
    pipe = IdentificationPipeline(g.robot(), g.param, params_std=g.params_std(), coupling=g.coupling, chunk_samples=chunk)
    pipe.set_samples(q, v, a)
    pipe.set_tau_from_parameters(g.phi_ref(), noise_std=0.05)
    out = pipe.run()
    assert out["rows"] == 6 * N and out["idx_base"] == list(g["idx_base"])
    assert seen and all(r == 6 * N for r, _ in seen)
    assert all(p == 6 * (-(-N // chunk) if chunk else 1) for _, p in seen)
    assert out["null_rule_certified"] and pipe.null_rule_fallbacks == 0
