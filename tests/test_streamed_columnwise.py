"""GPU suite: the streamed entry points -- figh_regressor_tsqr, figh_regressor_tsqr_norms, figh_regressor_gram
(csrc/figh_stream.hip, regressor_tsqr_impl) -- column by column through every branch of their chunk loop.

The QR kernels are checked column by column on exact inputs (test_qr_graded.py, test_qr_structured_graded.py) and the
regressor kernels entry by entry (test_regressor_entrywise.py); this file gives the host loop that joins them the same
standard.  A wrong branch there faults nothing: it drops or double-counts rows and returns a slightly wrong R.

Reference: the W figh_regressor_build writes for all N samples in one call (reference layout, read back), A = [W[:, cols]
| tau] with its rows scaled by the weights, and the Gram of A in long double (own error rows 2^-64, asserted to be a tenth
of the tolerance).  Per case (stream_common.CASES; test_streamed_plan_host.py shows that the table reaches every branch):

* R == triu(R) and the column-wise backward metric max |R^T R - G|_ij / (|a_i| |a_j|) <= qr_graded_common.TOL_BACKWARD;
* the diagonal metric (C_DIAG cond u) where the long-double Cholesky factor is a valid reference, else the set
  {k : |R_kk| > 1e-8} against plain Householder QR of A on the host; listed zero columns give zero columns of R;
* the norms of figh_regressor_tsqr_norms from the same call, within gamma_m + SIBLING_SLACK (test_reductions_graded.py);
* figh_regressor_gram by the three entrywise bounds of test_reductions_graded.test_regressor_gram_entrywise;
* the null-pivot rule over chunks by qr_graded_common.null_rule_check with pieces = rows per sample x chunks;
* the launches the profiling counters show ("tsqr" + "tsqr_small", "regressor_chain" + "regressor_tree") against the plan.

Not covered here: multi-workgroup chains of the widest geometries (TALOS' 331 and the SIP program's 400 columns, 21 and 25
column chunks).  Their reference needs about 1e9 long-double multiply-adds per case; they keep the one-workgroup chains of
test_qr_graded.test_streamed_regressor_tsqr_columnwise.  The chains of several workgroups are carried by the geometries of
up to 6 column chunks (81 .. 97 columns) and TIAGo's 180 columns.

Measured on an MI355X (tolerance 1e-13), largest backward metric per group: a (chunk shapes) 9.9e-16, b (hinted tree)
1.8e-15, c (chains of 2 and 4 workgroups) 2.4e-15, d (split) 2.5e-15, e (link-compact and fallback) 7.6e-15, f (tile-blocked
inputs) 1.6e-15, g (null-pivot rule) 1.7e-15.  Diagonal metric at most 0.94 cond u (tolerance 200), norms 5.1e-4 of their
bound, figh_regressor_gram 2.6e-2 TOL_BACKWARD, the null rule's bound used to 2.1e-4 (rule on) and 1.7e-2 (off); tile-blocked
and sample-major inputs gave bit-identical R, and so did the repeated call of the carried-state test.  The module takes
about 8 s, no case more than 1 s.
"""
import functools

import numpy as np
import pytest

import qr_graded_common as qg
import reductions_common as rc
import stream_common as sc
from test_qr_graded import C_DIAG, TOL_QR, U
from test_reductions_graded import SIBLING_SLACK

pytestmark = pytest.mark.gpu

TOL_BACKWARD = qg.TOL_BACKWARD
COND_MAX = 0.1 * U / 2.0 ** -64  # the guard of test_qr_graded._check: cond^2 2^-64 <= 0.1 cond u


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    qg.check_longdouble()
    return _lib


# ------------------------------------------------------------------------------------------------------------ reference
@functools.lru_cache(maxsize=3)
def _samples_and_W(model, param_key, N):
    """(device q, v, a, host q, v, a, reference-layout W of figh_regressor_build for all N samples in one call)."""
    from figaroh_plus_amd import _lib
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    from figaroh_plus_amd.tools.regressor import _samples_to_device
    case = next(c for c in sc.CASES if (c.model, c.param, c.N) == (model, param_key, N))
    param, coupling = sc.case_param(case)
    robot = sc.robot_of(model)
    mode, flags, ft = sc.call_flags(param, coupling, 0)
    h = robot.device_model()
    rps, ncols = h.shape(mode, flags)
    q, v, a = sample_inputs(robot.model, N, np.random.default_rng([N, len(model), 3]), 1.5, 2, 5)
    _, d_q, d_v, d_a = _samples_to_device(robot.model, q, v, a)
    d_W = _lib.DeviceArray((rps * N * ncols,))
    _lib.regressor_build(h, mode, flags, ft, N, d_q, d_v, d_a, d_W, ncols, None)
    W = d_W.to_host().reshape(rps * N, ncols)
    d_W.free()
    return (d_q, d_v, d_a), W


class Problem:
    """One case: its inputs on the device, A (weighted), tau and the long-double Gram."""

    def __init__(self, case):
        self.case = case
        self.param, self.coupling = sc.case_param(case)
        self.robot = sc.robot_of(case.model)
        self.mode, self.flags, self.ft = sc.call_flags(self.param, self.coupling, 0)
        self.plan = sc.case_plan(case)
        self.dev, W = _samples_and_W(case.model, case.param, case.N)
        self.rows, self.ncols = W.shape
        self.rps = self.rows // case.N
        f = sc.facts(case.model, self.param, self.coupling)
        assert (self.rps, self.ncols) == (f.rps, f.ncols)
        self.cols = sc.column_list(case)
        self.n = len(self.cols)
        rng = np.random.default_rng([case.N, self.n, 11])
        A = W[:, self.cols]
        self.tau = None
        if case.with_tau:
            scale = np.sqrt((A * A).sum(axis=0))
            x = rng.standard_normal(self.n) / np.where(scale > 0, scale, 1.0) * np.sqrt(self.rows)
            # (noise a quarter of the signal: tau must not be nearly dependent, or no case has a well-conditioned reference)
            self.tau = A @ x + 0.25 * np.sqrt(self.n) * rng.standard_normal(self.rows)
            A = np.c_[A, self.tau]
        if case.weights is not None:
            w = np.asarray(case.weights, dtype=np.float64)
            assert self.rps % len(w) == 0
            A = A * np.repeat(w, self.rows // len(w))[:, None]
        self.A = A
        self.nc = A.shape[1]
        assert self.nc == self.plan.nc
        # the reference's own column-wise error, rows 2^-64, must stay a tenth of the tolerance (_check_against_W)
        assert self.rows * 2.0 ** -64 <= 0.1 * TOL_BACKWARD
        Al = np.asarray(A, dtype=np.longdouble)
        self.G = Al.T @ Al
        self.colsq_ref = rc.colsq_ld(W) if sc.ENTRY.get(case.id) == "norms" else None

    def inputs(self, lib, blocked):
        if not blocked:
            return self.dev
        m = self.robot.model
        return tuple(lib.repack_samples(d, self.case.N, w) for d, w in zip(self.dev, (m.nq, m.nv, m.nv)))


@functools.lru_cache(maxsize=2)
def _problem(case_id):
    return Problem(sc.CASE[case_id])


def _launches(lib, names):
    return sum(lib.profile_get(nm)[0] for nm in names)


def _run(lib, pb, entry="tsqr", blocked=False):
    """One call of the entry under profiling level 2: (R or None, colsq or None, gram or None, level-0 launches, regressor
    launches)."""
    case = pb.case
    d_q, d_v, d_a = pb.inputs(lib, blocked)
    flags = pb.flags | (lib.FLAG_BLOCKED_INPUTS if blocked else 0)
    d_idx = lib.DeviceArray.from_host(pb.cols)
    d_tau = lib.DeviceArray.from_host(pb.tau) if pb.tau is not None else None
    h = pb.robot.device_model()
    R = cs = gram = None
    lib.profile_enable(True, 2)
    try:
        lib.profile_reset()
        if entry == "gram":
            gram = lib.regressor_gram(h, pb.mode, flags, pb.ft, case.N, d_q, d_v, d_a, d_idx, pb.n, d_tau, case.chunk)
        else:
            d_R = lib.DeviceArray.from_host(np.full(pb.nc * pb.nc, np.nan))
            d_cs = lib.DeviceArray.from_host(np.full(pb.ncols, np.nan)) if entry == "norms" else None
            lib.regressor_tsqr(h, pb.mode, flags, pb.ft, case.N, d_q, d_v, d_a, d_idx, pb.n, d_tau, case.weights, d_R,
                               chunk_samples=case.chunk, d_colsq=d_cs)
            R = d_R.to_host().reshape(pb.nc, pb.nc)
            cs = d_cs.to_host() if d_cs is not None else None
        lib.synchronize()
        level0 = _launches(lib, ("tsqr", "tsqr_small"))
        regs = _launches(lib, ("regressor_chain", "regressor_tree"))
    finally:
        lib.profile_enable(False)
    return R, cs, gram, level0, regs


def _backward(R, G):
    assert np.array_equal(R, np.triu(R)), "R is not upper triangular"
    return qg.backward_err(R, G)


def _reference_base(pb):
    """{k < n : |R_kk| > tol_qr} of plain Householder QR of A on the host (np.linalg.qr: the reference's own decision,
    qrdecomposition.py:205-221); every pivot a factor 3 away from the threshold, so that rounding cannot move it."""
    d = np.abs(np.diag(np.linalg.qr(pb.A, mode="r")))[:pb.n]
    assert not np.any((d > TOL_QR / 3) & (d < 3 * TOL_QR)), "a reference pivot too close to tol_qr: choose another case"
    return np.flatnonzero(d > TOL_QR).tolist()


def _check_R(R, pb, record_property, tag):
    b = _backward(R, pb.G)
    record_property(tag + ":backward", "%.3e" % b)
    print("streamed %-28s backward %.3e" % (tag, b))
    assert b <= TOL_BACKWARD, "%s: backward %.3e > %.1e" % (tag, b, TOL_BACKWARD)
    dead = [int(np.flatnonzero(pb.cols == c)[0]) for c in sc.DEAD_COLUMNS.get(pb.case.id, [])]
    for k in dead:  # exact zero columns stay exact zeros
        assert not pb.A[:, k].any() and not R[:, k].any(), "%s: listed zero column %d" % (tag, k)
    full = False
    try:
        R_ref = qg.cholesky_ld(pb.G)
        cond = qg.equilibrated_cond(R_ref)
        full = np.isfinite(cond) and cond <= COND_MAX
    except np.linalg.LinAlgError:
        pass
    record_property(tag + ":full_rank_reference", str(bool(full)))
    assert full or pb.case.id not in sc.FULL_RANK, "%s: meant to be checked against the Cholesky factor" % tag
    if full:
        d = qg.diag_err(R, R_ref, pb.G)
        record_property(tag + ":diag_over_cond_u", "%.3e" % (d / (cond * U)))
        assert d <= C_DIAG * cond * U, "%s: diagonal %.3e > %g cond u (cond %.3g)" % (tag, d, C_DIAG, cond)
    else:
        base = _reference_base(pb)
        got = np.flatnonzero(np.abs(np.diag(R))[:pb.n] > TOL_QR).tolist()
        assert got == base, "%s: base set differs from the reference's" % tag
        assert not set(dead) & set(got)
    return b


def _check_path(pb, level0, regs, tag):
    assert level0 == pb.plan.level0_launches, "%s: %d level-0 launches, plan %d" % (tag, level0, pb.plan.level0_launches)
    assert regs == pb.plan.nchunks, "%s: %d regressor launches, %d chunks" % (tag, regs, pb.plan.nchunks)


# ---------------------------------------------------------------------------------------------------------------- cases
@pytest.mark.parametrize("case_id", [c.id for c in sc.CASES])
def test_streamed_case_columnwise(lib, case_id, record_property):
    """Every case of stream_common.CASES through its entry: R (or the Gram terms), the norms of the same call, the rank
    decision and the launches against the plan.  Tile-blocked cases run the sample-major call as well; both are checked."""
    pb = _problem(case_id)
    case, plan = pb.case, pb.plan
    entry = sc.ENTRY.get(case_id, "tsqr")
    record_property("plan", str(plan._asdict()))
    blocked = bool(case.flags & sc.FLAG_BLOCKED_INPUTS)
    R, cs, gram, level0, regs = _run(lib, pb, entry, blocked)
    _check_path(pb, level0, regs, case_id)
    if entry == "gram":
        n = pb.n
        nrm = np.sqrt(np.asarray(np.diag(pb.G), dtype=np.float64))
        G, gv, tt = gram
        EG = np.abs(np.asarray(G, dtype=np.longdouble) - pb.G[:n, :n]) / np.outer(nrm[:n], nrm[:n])
        Eg = np.abs(np.asarray(gv, dtype=np.longdouble) - pb.G[:n, n]) / (nrm[:n] * nrm[n])
        Et = abs(np.longdouble(tt) - pb.G[n, n]) / pb.G[n, n]
        w = float(max(EG.max(), Eg.max(), Et)) / TOL_BACKWARD
        record_property(case_id + ":gram_over_bound", "%.3e" % w)
        print("streamed %-28s gram %.3e TOL_BACKWARD" % (case_id, w))
        assert float(EG.max()) <= TOL_BACKWARD and float(Eg.max()) <= TOL_BACKWARD and float(Et) <= TOL_BACKWARD
        return
    _check_R(R, pb, record_property, case_id)
    if entry == "norms":
        r = rc.colsq_ratio(cs, pb.colsq_ref, pb.rows, SIBLING_SLACK)
        record_property(case_id + ":norms_over_bound", "%.3e" % float(np.max(r, initial=0.0)))
        bad = np.flatnonzero(~(r <= 1.0))
        assert bad.size == 0, "%s: column norms %s off their reference" % (case_id, bad[:8].tolist())
    if blocked:
        R2, _, _, level0, regs = _run(lib, pb, entry, False)
        _check_path(pb, level0, regs, case_id + "/sample-major")
        _check_R(R2, pb, record_property, case_id + "/sample-major")
        record_property(case_id + ":blocked_equals_sample_major", str(bool(np.array_equal(R, R2))))


def test_blocked_inputs_refused_for_ragged_tiles(lib):
    """Tile-blocked inputs with chunk_samples = 150 and more than one chunk: FIGH_ERR_INVALID, d_R untouched."""
    pb = _problem("f_blocked")
    d_q, d_v, d_a = pb.inputs(lib, True)
    d_idx = lib.DeviceArray.from_host(pb.cols)
    d_tau = lib.DeviceArray.from_host(pb.tau)
    d_R = lib.DeviceArray.from_host(np.full(pb.nc * pb.nc, -7.0))
    h = pb.robot.device_model()
    args = (h.handle, pb.mode, pb.flags | lib.FLAG_BLOCKED_INPUTS, pb.ft, pb.case.N, d_q.ptr, d_v.ptr, d_a.ptr, d_idx.ptr,
            pb.n, d_tau.ptr, None, 0)
    assert lib.load().figh_regressor_tsqr(*args, 150, d_R.ptr) == lib.ERR_INVALID
    assert np.all(d_R.to_host() == -7.0)
    # one chunk of any size is accepted
    assert lib.load().figh_regressor_tsqr(*args, pb.case.N, d_R.ptr) == lib.FIGH_OK
    R = d_R.to_host().reshape(pb.nc, pb.nc)
    assert _backward(R, pb.G) <= TOL_BACKWARD


# ------------------------------------------------------------------------------------------------------- null-pivot rule
@pytest.mark.parametrize("case_id", ["g_ur10", "g_split"])
def test_null_pivot_rule_over_chunks(lib, case_id, record_property):
    """The null-pivot rule in a chunked call: the column bound of qr_graded_common.null_rule_check with pieces = rows per
    sample x chunks, the base set that of plain Householder QR with the rule on and off."""
    pb = _problem(case_id)
    base = _reference_base(pb)
    assert len(base) < pb.n, "the list has no dependent columns"
    got = {}
    for rule in (False, True):
        with lib.null_pivots(TOL_QR if rule else 0.0):
            R, _, _, level0, regs = _run(lib, pb)
        _check_path(pb, level0, regs, case_id)
        assert np.array_equal(R, np.triu(R))
        qg.null_rule_check(R, pb.G, pb.rows, pb.plan.pieces, base, pb.n, "null_streamed_%s_%d" % (case_id, rule),
                           record_property, rule)
        got[rule] = np.flatnonzero(np.abs(np.diag(R))[:pb.n] > TOL_QR).tolist()
    assert got[False] == got[True] == base


# ---------------------------------------------------------------------------------------------------------- carried state
def test_hint_cache_across_models_and_chunk_heights(lib, record_property):
    """tile_hint keeps its per-tile table from call to call, keyed on (buffer, rows, first columns); a ragged run alternates
    between two chunk heights.  Case A (fork, hinted, ragged), then B (UR10, hinted), then A again in one process."""
    A, B = _problem("b_sorted"), _problem("a_ragged")
    assert all(A.plan.hinted) and all(B.plan.hinted) and A.plan.last != A.plan.cs
    R1 = _run(lib, A)[0]
    Rb = _run(lib, B)[0]
    R2 = _run(lib, A)[0]
    for tag, R, pb in (("A_first", R1, A), ("B", Rb, B), ("A_again", R2, A)):
        b = _backward(R, pb.G)
        record_property("carried_%s:backward" % tag, "%.3e" % b)
        assert b <= TOL_BACKWARD, "%s: backward %.3e" % (tag, b)
    record_property("carried:A_bit_identical", str(bool(np.array_equal(R1, R2))))


# -------------------------------------------------------------------------------------------------------- argument checks
def test_argument_checks_launch_nothing(lib):
    """Refused calls return FIGH_ERR_INVALID before anything is launched (d_R keeps its sentinel, no kernel counted);
    N = 0 gives FIGH_OK, R = 0 and zero norms."""
    pb = _problem("a_ragged")
    d_q, d_v, d_a = pb.dev
    h = pb.robot.device_model()
    d_idx = lib.DeviceArray.from_host(np.arange(pb.ncols + 1, dtype=np.int32) % pb.ncols)
    nmax = pb.ncols + 2
    d_R = lib.DeviceArray.from_host(np.full(nmax * nmax, -7.0))
    d_cs = lib.DeviceArray.from_host(np.full(pb.ncols, -7.0))
    w3 = np.ones(4)  # 4 does not divide the 6 rows of a sample
    wp = w3.ctypes.data_as(lib._c_double_p)
    L = lib.load()
    head = (h.handle, pb.mode, pb.flags, pb.ft, pb.case.N, d_q.ptr, d_v.ptr, d_a.ptr)
    bad = [
        head + (d_idx.ptr, pb.ncols + 1, None, None, 0, 64),   # n > ncols
        head + (None, pb.ncols - 1, None, None, 0, 64),        # NULL list with n != ncols
        head + (d_idx.ptr, 10, None, wp, 4, 64),               # nblocks does not divide rps
        head + (d_idx.ptr, 10, None, None, 0, -64),            # negative chunk_samples
    ]
    lib.profile_enable(True, 2)
    try:
        lib.profile_reset()
        for args in bad:
            assert L.figh_regressor_tsqr(*args, d_R.ptr) == lib.ERR_INVALID
            assert L.figh_regressor_tsqr_norms(*args, d_R.ptr, d_cs.ptr) == lib.ERR_INVALID
        lib.synchronize()
        for nm in ("tsqr", "tsqr_small", "regressor_chain", "regressor_tree"):
            assert lib.profile_get(nm)[0] == 0
    finally:
        lib.profile_enable(False)
    assert np.all(d_R.to_host() == -7.0) and np.all(d_cs.to_host() == -7.0)
    # N = 0
    zero = (h.handle, pb.mode, pb.flags, pb.ft, 0, d_q.ptr, d_v.ptr, d_a.ptr, d_idx.ptr, 10, None, None, 0, 64)
    assert L.figh_regressor_tsqr(*zero, d_R.ptr) == lib.FIGH_OK
    out = d_R.to_host()
    assert not out[:100].any() and np.all(out[100:] == -7.0)
    d_R2 = lib.DeviceArray.from_host(np.full(100, -7.0))
    assert L.figh_regressor_tsqr_norms(*zero, d_R2.ptr, d_cs.ptr) == lib.FIGH_OK
    assert not d_R2.to_host().any() and not d_cs.to_host().any()
