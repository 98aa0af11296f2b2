"""GPU suite: libfigh's carried state between calls, from a known state.

Every other suite tests a call as if it were the only call of the process; a stale per-tile hint, a stale entry in a
buffer of the streamed merge tree or a workspace slot two users grow would not fault -- each gives a plausible, wrong R.
Here each family of tests/call_sequence_common.py runs as ONE sequence in ONE fresh process (call_sequence_worker.py: empty
slots, cold caches), and every step's raw result is judged here with the metric and the tolerance its entry has in the
existing suites (test_qr_graded._check, test_qr_structured_graded, reductions_common, regressor_exact, the filter's float64
mirror): imported, not copied.  A step that repeats an earlier call must satisfy the same metric; bits are compared only
where figh.h documents reproducibility or the suite already compares with a mirror (W, the filter output).  Everywhere
else the test records whether the repeat was bit-equal (``<tag>:bit_equal``) without asserting it.

One worker at a time.  A worker that ends with a signal, a non-zero status or its time limit fails its family with its
output, and the remaining families then fail at once without starting another GPU process.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import call_sequence_common as cs
import preprocessing_common as pc
import qr_graded_common as qg
import reductions_common as rc
import regressor_exact as rx
from test_qr_graded import TOL_BACKWARD, _check, _check_against_W, _fold_term
from test_qr_structured_graded import _check_gram
from test_reductions_graded import SIBLING_SLACK

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER_TIMEOUT = 300  # a safety cap (the existing worker tests allow 500 to 900 s), not a measurement: a family takes seconds
_BROKEN = []  # the family whose worker faulted, hung or failed: no further GPU process is started after it


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(np.uint8), b.view(np.uint8)))


def _no_sentinel(x, what):
    assert not (np.asarray(x) == cs.SENT).any(), "%s: an element of the result was never written" % what


def _upper(R, what):
    """The upper triangle of an nc x nc result (what the entries define; the mirrors of qrdecomposition.py read no more)."""
    R = np.triu(R)
    _no_sentinel(R, what)
    return R


# ------------------------------------------------------------------------------------------------ the metric of each op
def check_tsqr(a, r, rp, tag):
    h = a["h"]
    _check(_upper(r["R"], tag), h.gram(), rp, tag, forward=h.forward())


def check_tsqr_selected(a, r, rp, tag):
    g = a["g"]
    sel = r["sel"]
    assert sel[0] == g.n and sel[2:2 + g.n].tolist() == g.kept.tolist(), "%s: kept columns differ" % tag
    _check(_upper(r["R"], tag), g.gram(), rp, tag)


def check_merge(a, r, rp, tag):  # test_qr_graded.test_merge_graded_columns
    g = a["g"]
    _no_sentinel(r["R"], tag)
    _check(r["R"], g.gram(), rp, tag)


def check_merge_base(a, r, rp, tag):  # test_qr_graded.test_merge_base_graded_exact_dependencies
    g = a["g"]
    n, nc, rows_k = g.n_free, g.nc, r["rows"]
    _no_sentinel(rows_k, tag)
    G = g.gram()
    base_n = g.base_free()
    R_ref = qg.cholesky_ld(G[np.ix_(base_n, base_n)])
    assert float(np.diag(R_ref).min()) >= 3 * cs.TOL_QR
    d = np.abs(rows_k[nc])
    assert np.flatnonzero(d[:n] > cs.TOL_QR).tolist() == base_n, "%s: base set differs from the exact one" % tag
    assert d[g.dep].max(initial=0.0) <= cs.TOL_QR / 3
    assert not rows_k[g.dep].any()
    _check(np.triu(rows_k[base_n][:, base_n]), G[np.ix_(base_n, base_n)], rp, tag + "_R1", R_ref=R_ref)
    _check(rows_k[base_n + list(range(n, nc))], G, rp, tag + "_rows", forward=False, triangular=False)


def check_filtfilt(a, r, rp, tag):  # test_preprocessing_exact._check_case: the float64 mirror, bit for bit
    x = a["x"]
    ref = pc.filtfilt_ref(a["form"], a["b"], a["a"], a["zi"], a["padlen"], a["q"], x, a["nblocks"])
    got = int(r["rows_out"])
    assert got == ref.shape[0], "%s: %d rows out, expected %d" % (tag, got, ref.shape[0])
    y = r["y"]
    assert (y[got:] == cs.SENT).all(), "%s: rows behind the result were written" % tag
    assert np.array_equal(y[:got], ref), "%s: %d samples differ from the float64 mirror" % (tag, int((y[:got] != ref).sum()))


def check_wrench(a, r, rp, tag):  # test_qr_structured_graded.test_wrench_graded_layouts, full rank
    g = a["g"]
    compact = a["layout"] == "force-link-compact"
    sel = r["sel"]
    want = qg.device_column(g.kept, 16, g.link_pos if compact else None)
    assert sel[0] == g.n and sel[2:2 + g.n].tolist() == want.tolist(), "%s: kept columns differ" % tag
    _check(_upper(r["R"], tag), g.gram(a["with_tau"]), rp, tag)


def check_blocks(a, r, rp, tag):  # test_qr_structured_graded.test_blocks_graded_full_rank
    g, with_tau = a["g"], a["with_tau"]
    n = g.n
    sel = r["sel"]
    assert sel[0] == n and sel[2:2 + n].tolist() == qg.device_column(g.kept, 16).tolist(), "%s: kept columns differ" % tag
    _check(_upper(r["R"], tag), g.gram(with_tau), rp, tag)
    if not a["want_tri"]:
        return
    S, off = r["stack"], g.stack_offsets(with_tau)
    _no_sentinel(S, tag + "_stack")
    for b in range(g.nblocks):
        if off[b + 1] == off[b]:
            continue
        L = np.r_[g.lists[b], [n] if with_tau else []].astype(np.int64)
        Sb = S[off[b]:off[b + 1]]
        assert not np.delete(Sb, L, axis=1).any(), "%s: block %d has entries outside its list" % (tag, b)
        _check(Sb[:, L], g.block_gram(b, with_tau), rp, "%s_stack_b%d" % (tag, b))


def check_fused(a, r, rp, tag):  # test_qr_graded.test_fused_chain_and_two_launch_columnwise + the producer's entries
    assert int(r["served"]) == 1, "%s: the fused launch did not serve a 6-joint chain at N = %d" % (tag, cs.UR10_FUSED_N)
    W, kept = r["W"], cs.fused_kept()
    _, ref = rx.reference("ur10", "unit", cs.UR10_FUSED_N, rx.base_param(), seed=4)
    rp(tag + ":entry_ratio", "%.2f" % rx.assert_entrywise(W, ref, rx.C_TOL, tag))
    ratio = rc.colsq_ratio(r["colsq_fused"], rc.colsq_ld(W), W.shape[0])
    rp(tag + ":colsq_over_bound", "%.3e" % float(ratio.max()))
    assert (ratio <= 1.0).all(), "%s: fused column norms off the sums of the W it wrote" % tag
    _check_against_W(_upper(r["R"], tag), np.c_[W[:, kept], a["tau"]], rp, tag)


_W_CACHE = {}


def _stream_W(model, results):
    """(W of the first STREAM_N samples, W of every batch trajectory) from the family's rbuild step: row block j of
    trajectory b is rows j N_tot + b STREAM_N + [0, STREAM_N)."""
    if model not in _W_CACHE:
        W = results["00_W_%s" % model]["W"]
        Nt, N = cs.stream_total(model), cs.STREAM_N
        rps = W.shape[0] // Nt
        trajs = [W[(np.arange(rps)[:, None] * Nt + b * N + np.arange(N)[None, :]).reshape(-1)] for b in range(Nt // N)]
        _W_CACHE[model] = trajs
    return _W_CACHE[model]


def check_rbuild(a, r, rp, tag):  # test_regressor_entrywise: the W every other step of the family is judged against
    model = a["model"]
    param, _, _ = cs.stream_inputs(model)
    _, ref = rx.reference(model, "unit", cs.stream_total(model), param, seed=6)
    rp(tag + ":entry_ratio", "%.2f" % rx.assert_entrywise(r["W"], ref, rx.C_TOL, tag))
    ratio = rc.colsq_ratio(r["colsq"], rc.colsq_ld(r["W"]), r["W"].shape[0])
    rp(tag + ":colsq_over_bound", "%.3e" % float(ratio.max()))
    assert (ratio <= 1.0).all(), "%s: column norms off the sums of the W it wrote" % tag


def _norms_ok(cs_dev, W, rp, tag):  # test_reductions_graded.test_norms_only_entries
    _no_sentinel(cs_dev, tag)
    ratio = rc.colsq_ratio(cs_dev, rc.colsq_ld(W), W.shape[0], SIBLING_SLACK)
    rp(tag + ":colsq_over_bound", "%.3e" % float(ratio.max()))
    bad = np.flatnonzero(~(ratio <= 1.0))
    assert bad.size == 0, "%s: columns %s off their reference" % (tag, bad[:8].tolist())


def check_rcolsq(a, r, rp, tag, results):
    _norms_ok(r["colsq"], _stream_W(a["model"], results)[0], rp, tag)


def check_rtsqr(a, r, rp, tag, results):
    W = _stream_W(a["model"], results)[0]
    kept, tau = cs.stream_kept(a["model"]), cs.stream_inputs(a["model"])[2]
    A = np.asarray(np.c_[W[:, kept], tau], dtype=np.longdouble)
    _check_gram(_upper(r["R"], tag), A.T @ A, rp, tag)
    if a["norms"]:
        _norms_ok(r["colsq"], W, rp, tag)


def check_rbatch(a, r, rp, tag, results):  # test_qr_structured_graded.test_regressor_tsqr_batch_columnwise
    kept = cs.stream_kept(a["model"])
    for b, W in enumerate(_stream_W(a["model"], results)):
        A = np.asarray(W[:, kept], dtype=np.longdouble)
        _check_gram(_upper(r["R"][b], tag), A.T @ A, rp, "%s_b%d" % (tag, b))


def check_rgram(a, r, rp, tag, results):  # test_reductions_graded.test_regressor_gram_entrywise
    W = _stream_W(a["model"], results)[0]
    kept, tau = cs.stream_kept(a["model"]), cs.stream_inputs(a["model"])[2]
    n = len(kept)
    A = np.asarray(np.c_[W[:, kept], tau], dtype=np.longdouble)
    Gl = A.T @ A
    nrm = np.sqrt(np.asarray(np.diag(Gl), dtype=np.float64))
    nrm = np.where(nrm > 0, nrm, 1.0)
    EG = np.abs(np.asarray(r["G"], dtype=np.longdouble) - Gl[:n, :n]) / np.outer(nrm[:n], nrm[:n])
    Eg = np.abs(np.asarray(r["g"], dtype=np.longdouble) - Gl[:n, n]) / (nrm[:n] * nrm[n])
    Et = abs(np.longdouble(float(r["tt"])) - Gl[n, n]) / Gl[n, n]
    w = float(max(EG.max(), Eg.max(), Et)) / TOL_BACKWARD
    rp(tag + ":gram_over_bound", "%.3e" % w)
    assert w <= 1.0, "%s: %.3g TOL_BACKWARD" % (tag, w)


def check_tsqr_deps(a, r, rp, tag):  # test_qr_graded.test_null_pivot_rule_graded_column_bound
    g, R = a["g"], _upper(r["R"], tag)
    G = g.gram()
    assert g.min_base_pivot() >= 3 * cs.TOL_QR
    assert np.flatnonzero(np.abs(np.diag(R)) > cs.TOL_QR).tolist() == g.base, "%s: base set differs" % tag
    nrm = np.where(qg.col_norms(G) > 0, qg.col_norms(G), 1.0)
    Rl = np.asarray(np.triu(R), dtype=np.longdouble)
    E = np.abs(Rl.T @ Rl - np.asarray(G, dtype=np.longdouble)) / np.outer(nrm, nrm).astype(np.longdouble)
    # rule off: the exact-zero rule folds nothing, the plain column-wise bound holds
    bound = TOL_BACKWARD + (_fold_term(G, g.rows) if a["rule"] else 0.0)
    rp(tag + ":backward_over_bound", "%.3e" % float((E / bound).max()))
    assert (E <= bound).all(), "%s: column-wise backward error above the bound (rule %s)" % (tag, a["rule"])


def check_build_profile(a, r, rp, tag):
    _, ref = rx.reference(a["model"], "unit", len(a["q"]), a["param"], seed=2)
    rp(tag + ":entry_ratio", "%.2f" % rx.assert_entrywise(r["W"], ref, rx.C_TOL, tag))


def check_active_rows_ab(a, r, rp, tag):
    _, ref = rx.reference(a["model"], "unit", len(a["q"]), a["param"], seed=2)
    N, nl = len(a["q"]), ref.W.shape[1] // 14
    c = np.arange(14 * nl)
    dev = 16 * (c // 14) + c % 14
    rp(tag + ":entry_ratio", "%.2f" % rx.assert_entrywise(r["W_B1"][:, dev], ref, rx.C_TOL, tag))
    for other in ("B2", "B3"):
        assert _bits_equal(r["W_B1"], r["W_" + other]), "%s: handle B's build %s differs from its first build" % (tag, other)
        assert _bits_equal(r["colsq_B1"], r["colsq_" + other]), "%s: handle B's norms %s differ" % (tag, other)
    stored = np.repeat(np.isin(np.arange(nl), a["rows_a"]), N)
    assert _bits_equal(r["W_A"][stored], r["W_B1"][stored]), "%s: handle A's stored blocks differ from a full build" % tag
    assert (r["W_A"][~stored] == cs.SENT).all(), "%s: handle A wrote a row block that is not active" % tag


CHECK = {"tsqr": check_tsqr, "tsqr_selected": check_tsqr_selected, "merge": check_merge, "merge_base": check_merge_base,
         "filtfilt": check_filtfilt, "wrench": check_wrench, "blocks": check_blocks, "fused": check_fused,
         "rbuild": check_rbuild, "rcolsq": check_rcolsq, "rtsqr": check_rtsqr, "rbatch": check_rbatch, "rgram": check_rgram,
         "tsqr_deps": check_tsqr_deps, "build_profile": check_build_profile, "active_rows_ab": check_active_rows_ab}
NEEDS_RESULTS = {"rcolsq", "rtsqr", "rbatch", "rgram"}  # judged against the W another step of the family read back


def _run_worker(family, out):
    if _BROKEN:
        pytest.fail("not started: the worker of family %r faulted, hung or failed earlier in this session" % _BROKEN[0])
    cmd = [sys.executable, os.path.join(HERE, "call_sequence_worker.py"), family, str(out)]
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=WORKER_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _BROKEN.append(family)
        pytest.fail("worker of family %r did not finish within %d s; output:\n%s" % (
            family, WORKER_TIMEOUT, (e.stdout or b"").decode(errors="replace")[-4000:]))
    if p.returncode != 0:
        _BROKEN.append(family)
        pytest.fail("worker of family %r ended with status %d; output:\n%s" % (
            family, p.returncode, p.stdout.decode(errors="replace")[-4000:]))
    z = np.load(str(out))
    results = {}
    for key in z.files:
        tag, name = key.split("/")
        results.setdefault(tag, {})[name] = z[key]
    return results


@pytest.mark.parametrize("family", cs.FAMILIES)
def test_call_sequence(family, tmp_path, record_property):
    """One family: the worker's sequence in a fresh process, then every step against its reference.  Every step is judged
    (a failing step does not hide the later ones); the failure message names family, step tag and metric."""
    qg.check_longdouble()
    table = cs.steps(family)
    results = _run_worker(family, tmp_path / (family + ".npz"))
    assert sorted(results) == sorted(s.tag for s in table), "the worker's results do not match the step table"
    failures = []
    for step in table:
        r = results[step.tag]
        try:
            if step.op in NEEDS_RESULTS:
                CHECK[step.op](step.args, r, record_property, step.tag, results)
            else:
                CHECK[step.op](step.args, r, record_property, step.tag)
        except AssertionError as e:
            failures.append("family %s, step %s (%s): %s" % (family, step.tag, step.op, e))
        if step.repeat_of is not None:
            first = results[step.repeat_of]
            for name in sorted(r):
                equal = _bits_equal(r[name], first[name])
                record_property("%s:bit_equal:%s" % (step.tag, name), str(equal))
                if name in step.bits and not equal:
                    failures.append("family %s, step %s: %s is not bit-equal to step %s" % (family, step.tag, name,
                                                                                           step.repeat_of))
    assert not failures, "\n".join(failures)
