"""GPU suite: column-wise accuracy of the structured TSQR entries on graded matrices with exact references.

test_qr_graded.py checks figh_tsqr, the merges and the kernel-built W column by column.  The structured entries -- the
wrench split (figh_tsqr_selected_wrench: force rows over their own columns, torque rows chained onto that triangle) and
the per-row-block factorisation (figh_tsqr_selected_blocks: grouped / mid / wide / plain blocks, the compact stack of
their embedded triangles, the single-workgroup factor of that stack and reveal_triangle) -- run TALOS, the human model
and TIAGo, and were checked only norm-wise.  Here they factor graded integer matrices with the zero structure these
entries exploit (tests/qr_graded_common.Wrench, RowBlocks), in every device layout they accept, against exact Grams and
their long-double Cholesky factors, with the metrics and tolerances of test_qr_graded.py.  The per-block stack, the
per-block residuals (figh_block_rows_residuals) and the weighted TSQR over that stack are checked block by block.
"""
import numpy as np
import pytest

import qr_graded_common as qg
from test_qr_graded import C_DIAG, PROFILES, TOL_BACKWARD, TOL_QR, U, _check

pytestmark = pytest.mark.gpu

NULL_TOL = TOL_QR / 64
# Largest values measured over this file on an MI355X (the tolerances are those of test_qr_graded.py): backward 4.8e-15
# (wrench, TALOS-like 330 columns, link-compact), forward 14.9 cond u and diagonal 14.8 cond u (same case), per-block stack
# backward 3.3e-15, weighted TSQR over the stack 8.0 cond u, null rule 0.037 of its bound, batched excitation TSQR
# backward 3.0e-15, the pipeline's own W through the entries 4.0e-15.
# |r^2_b - ||e_b||^2| <= C_R2 u (sum_c |v_c| |a_b,c|)^2 -- v^T (S^T S - G_b) v of a stack with a column-wise backward
# error, plus the residual kernel's rounding: measured 13.0 (wide blocks, exact dependencies, block-compact W)
C_R2 = 200.0


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    qg.check_longdouble()
    return _lib


def _forward_ok(G):
    """The long-double reference is accurate enough for the forward / diagonal metrics (full rank, moderate cond)."""
    try:
        R_ref = qg.cholesky_ld(G)
    except np.linalg.LinAlgError:
        return None
    cond = qg.equilibrated_cond(R_ref)
    return R_ref if cond * cond * 2.0 ** -64 <= 0.1 * cond * U else None


def _check_regrouped(rows_k, G, n, with_tau, base, dep, record_property, tag, R_plain=None):
    """The tol_qr >= 0 outputs (figh.h, figh_tsqr_selected): the base set is the exact one, dependent rows are zero, R1 and
    the base rows of [W1 W2 tau] against the exact factor / Gram, the residual against the exact one relative to |tau|
    (the tau column of the factor of [W_base tau]), row nc the plain diagonal."""
    nc = n + (1 if with_tau else 0)
    d = np.abs(rows_k[nc])
    assert np.flatnonzero(d[:n] > TOL_QR).tolist() == list(base), "%s: base set differs from the exact one" % tag
    assert d[dep].max(initial=0.0) <= TOL_QR / 3
    assert not rows_k[dep].any()
    R1_ref = qg.cholesky_ld(G[np.ix_(base, base)])
    assert float(np.diag(R1_ref).min()) >= 3 * TOL_QR  # the exact decision does not depend on rounding
    _check(np.triu(rows_k[base][:, base]), G[np.ix_(base, base)], record_property, tag + "_R1", R_ref=R1_ref)
    keep = list(base) + ([n] if with_tau else [])
    _check(rows_k[keep], G, record_property, tag + "_rows", forward=False, triangular=False)
    if with_tau:  # R1, Q1^T tau and the residual out[n][n] as one triangle: forward / diagonal of the tau column too
        # (the tau row's entries left of the diagonal are rounding residue, not exact zeros, on the narrow path)
        _check(rows_k[np.ix_(keep, keep)], G[np.ix_(keep, keep)], record_property, tag + "_residual", triangular=False)
    if R_plain is not None:  # row nc: the diagonal of the plain factorisation (tol_qr < 0) of the same matrix
        cond = qg.equilibrated_cond(R1_ref)
        nrm = np.where(qg.col_norms(G) > 0, qg.col_norms(G), 1.0)[:nc]
        dd = float((np.abs(d - np.abs(np.diag(R_plain))) / nrm).max())
        record_property(tag + ":plain_diag_over_cond_u", "%.3e" % (dd / (cond * U)))
        assert dd <= C_DIAG * cond * U


# ---------------------------------------------------------------------------------------------------- wrench entry
WRENCH_LAYOUTS = ["reference", "link-padded", "link-compact", "force-compact", "force-link-compact"]


def _wrench_buffers(g, layout):
    """(flat W, ldw, link_stride, link_pos or None, ld_force) of a layout."""
    if layout == "reference":
        return g.reference(), g.ncols, 14, None, 0
    if layout in ("link-padded", "link-compact"):
        W = g.padded(compact=layout == "link-compact")
        return W, W.shape[1], 16, g.link_pos if layout == "link-compact" else None, 0
    compact = layout == "force-link-compact"
    buf, ldw = g.force_compact(compact)
    return buf, ldw, 16, g.link_pos if compact else None, g.force_ld(compact)


def _run_wrench(lib, g, layout, with_tau, tol_qr, nf=None):
    buf, ldw, stride, pos, ldf = _wrench_buffers(g, layout)
    n = g.n
    nc = n + (1 if with_tau else 0)
    cs = g.colsq()
    tol_e = 0.5 * cs[cs > 0].min()
    d_sel = lib.DeviceArray((2 + 2 * g.ncols,), np.int32)
    d_R = lib.DeviceArray(((nc + 1) * nc,))
    lib.tsqr_selected_wrench(lib.DeviceArray.from_host(buf.reshape(-1)), g.rows, ldw, lib.DeviceArray.from_host(cs), g.ncols,
                             tol_e, stride, n, g.nf if nf is None else nf,
                             lib.DeviceArray.from_host(g.tau()) if with_tau else None, tol_qr, d_sel, d_R,
                             d_link_pos=lib.DeviceArray.from_host(pos) if pos is not None else None, ld_force=ldf)
    sel = d_sel.to_host()
    assert sel[0] == n and sel[2:2 + n].tolist() == qg.device_column(g.kept, stride, pos).tolist()
    out = d_R.to_host()
    return out[:nc * nc].reshape(nc, nc) if tol_qr < 0 else out.reshape(nc + 1, nc)


# (id, Nb, nlinks, n, dead links, extra slots, tau, profile): nc = n + tau just above the 80-column split threshold, human-
# like (ragged Nb, not a multiple of 64, rows / 2 >= 16 nc) and TALOS-like
WRENCH_CASES = [
    ("nc81", 450, 9, 80, (), False, True, "tiago"),
    ("nc82", 470, 10, 81, (3,), False, True, "wide"),
    ("nc82_notau", 470, 9, 82, (), True, False, "tiago"),
    ("human", 1031, 24, 189, (2, 9, 15, 20), False, True, "wide"),
    ("talos", 1792, 40, 329, (7,), False, True, "tiago"),
    ("talos_extra", 1800, 30, 330, (), True, False, "wide"),
]


@pytest.mark.parametrize("deps", [False, True])
@pytest.mark.parametrize("case", WRENCH_CASES, ids=[c[0] for c in WRENCH_CASES])
def test_wrench_graded_layouts(lib, case, deps, record_property):
    """figh_tsqr_selected_wrench in every layout the generator's columns allow.  Full rank: the plain triangle (tol_qr < 0)
    with all three metrics.  Exact dependencies: backward for the plain triangle, then tol_qr = 1e-8 -- the exact base set,
    zero dependent rows, R1, the base rows, the residual and the plain diagonal."""
    name, Nb, nlinks, n, dead, extra, with_tau, profile = case
    assert 3 * Nb >= 16 * (n + with_tau)  # the split runs
    rng = np.random.default_rng([Nb, n, int(deps), len(profile)])
    g = qg.Wrench(rng, Nb, nlinks, n, *PROFILES[profile], dead_links=dead, extra_slots=extra, deps=deps)
    assert 0 < g.nf < g.n
    G = g.gram(with_tau)
    R_ref = None if deps else qg.cholesky_ld(G)
    layouts = WRENCH_LAYOUTS if not extra else WRENCH_LAYOUTS[:3]
    for layout in layouts:
        tag = "wrench_%s_%s" % (name, layout)
        R = _run_wrench(lib, g, layout, with_tau, -1.0)
        _check(np.triu(R), G, record_property, tag, forward=not deps, R_ref=R_ref)
        if deps:
            rows_k = _run_wrench(lib, g, layout, with_tau, TOL_QR)
            _check_regrouped(rows_k, G, n, with_tau, [k for k in g.base if k < n], g.dep, record_property, tag, R_plain=R)


@pytest.mark.parametrize("case", ["nf0", "nc80", "short"])
def test_wrench_graded_fallbacks(lib, case, record_property):
    """The entry's fall-backs to the plain pass -- nf_expected = 0, at most 80 columns, rows / 2 < 16 nc -- column-wise in
    the layouts that allow them; a force-compact W refuses them (FIGH_ERR_UNSUPPORTED)."""
    Nb, nlinks, n, dead = {"nf0": (470, 10, 81, (3,)), "nc80": (400, 9, 79, ()), "short": (300, 12, 100, (4,))}[case]
    rng = np.random.default_rng([Nb, n, 99])
    g = qg.Wrench(rng, Nb, nlinks, n, *PROFILES["wide"], dead_links=dead, extra_slots=False)
    G = g.gram()
    R_ref = qg.cholesky_ld(G)
    nf = 0 if case == "nf0" else None
    for layout in WRENCH_LAYOUTS[:3]:
        R = _run_wrench(lib, g, layout, True, -1.0, nf=nf)
        _check(np.triu(R), G, record_property, "wrench_fallback_%s_%s" % (case, layout), R_ref=R_ref)
    for layout in WRENCH_LAYOUTS[3:]:
        with pytest.raises(lib.FighError) as err:
            _run_wrench(lib, g, layout, True, -1.0, nf=nf)
        assert err.value.code == lib.ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------- row-block entry
# groups of columns (size, blocks that list them); with tau, ncj = n_j + 1.
# WIDE_SPEC (nc 296 > 80: the stack goes through the single-workgroup factor and reveal_triangle): blocks 0-3 grouped
# (n_j 1, 63 -> ncj 64, 20, 40; rows_b >= 4096), 4-5 MID (ncj 65, 80), 6-7 WIDE (ncj 81, 200), 8 tau only, 9 inactive.
WIDE_SPEC = dict(nblocks=10, inactive=[9], k_block=7, noise={0: "tiny", 3: "tiny", 7: "big"},
                 groups=[(1, range(8)), (19, range(1, 8)), (43, [1]), (20, [3]), (30, [4, 5, 6, 7]), (14, [4]),
                         (20, [5, 6, 7]), (9, [5]), (10, [6]), (129, [7])])
# NARROW_SPEC (nc 80: the stack through the level-0 kernel and tsqr_reduce_stack): grouped n_j 1, 63, 20, 35; MID ncj 65,
# 80; 6 tau only; 7 inactive
NARROW_SPEC = dict(nblocks=8, inactive=[7], k_block=None, noise={0: "tiny", 2: "big"},
                   groups=[(1, range(6)), (19, range(1, 6)), (43, [1, 4, 5]), (1, [4, 5]), (15, [3, 5])])
# PLAIN_SPEC (no grouped launch: rows_b < 4096; no tau): plain n_j 5, 35, WIDE 95, a block with nothing kept, inactive
PLAIN_SPEC = dict(nblocks=5, inactive=[4], k_block=None, noise={},
                  groups=[(5, [0, 1, 2]), (30, [1, 2]), (60, [2])])
BLOCK_CASES = [("wide", WIDE_SPEC, 4096, True), ("narrow", NARROW_SPEC, 4096, True), ("plain", PLAIN_SPEC, 1000, False)]


def _row_blocks(spec, rows_b, profile, deps, seed):
    rng = np.random.default_rng(seed)
    return qg.RowBlocks(rng, rows_b, spec["nblocks"], spec["groups"], *PROFILES[profile], inactive=spec["inactive"],
                        deps=deps, noise=spec["noise"], k_block=spec["k_block"])


def _run_blocks(lib, g, compact, with_tau, tol_qr, want_tri):
    n = g.n
    nc = n + (1 if with_tau else 0)
    cs = g.colsq()
    tol_e = 0.5 * cs[cs > 0].min()
    counts, cols, pos = g.block_columns(16)
    off = ld = None
    if compact:
        buf, off, ld, cols = g.compact()
        rows_w = 1
    else:
        buf = g.dense(16)
        rows_w = buf.shape[1]
    d_sel = lib.DeviceArray((2 + 2 * g.ncols,), np.int32)
    d_R = lib.DeviceArray(((nc + 1) * nc,))
    d_tri = lib.DeviceArray(((int(g.stack_offsets(with_tau)[-1]) + nc + 1) * nc,)) if want_tri else None
    lib.tsqr_selected_blocks(lib.DeviceArray.from_host(buf.reshape(-1)), g.rows, rows_w, lib.DeviceArray.from_host(cs),
                             g.ncols, tol_e, 16, n, counts, lib.DeviceArray.from_host(cols),
                             lib.DeviceArray.from_host(pos), lib.DeviceArray.from_host(g.tau()) if with_tau else None,
                             tol_qr, d_sel, d_R, block_off=off, block_ld=ld, d_block_tri=d_tri)
    sel = d_sel.to_host()
    assert sel[0] == n and sel[2:2 + n].tolist() == qg.device_column(g.kept, 16).tolist()
    out = d_R.to_host()
    R = out[:nc * nc].reshape(nc, nc) if tol_qr < 0 else out.reshape(nc + 1, nc)
    return R, d_tri


def _check_stack(lib, g, d_tri, with_tau, deps, record_property, tag):
    """Each block's rows of the compact stack against the exact Gram of its [W_j[:, list_j] tau_j]; the stack holds exactly
    sum (n_j + 1) rows in block order, zero outside every block's list.  Then figh_block_rows_residuals on it against
    ||e_b||^2 per block.  Returns the stack."""
    n = g.n
    nc = n + (1 if with_tau else 0)
    off = g.stack_offsets(with_tau)
    S = d_tri.to_host()[:int(off[-1]) * nc].reshape(-1, nc)
    worst_r2 = 0.0
    for b in range(g.nblocks):
        if off[b + 1] == off[b]:
            continue
        L = np.r_[g.lists[b], [n] if with_tau else []].astype(np.int64)
        Sb = S[off[b]:off[b + 1]]
        assert not np.delete(Sb, L, axis=1).any(), "%s: block %d has entries outside its list" % (tag, b)
        Gb = g.block_gram(b, with_tau)
        ref = None if deps else _forward_ok(Gb)
        # (full-rank specs: every block's reference is good enough for the forward / diagonal metrics -- none is skipped)
        assert deps or ref is not None, "%s: block %d too ill-conditioned for the forward reference" % (tag, b)
        _check(Sb[:, L], Gb, record_property, "%s_stack_b%d" % (tag, b), forward=ref is not None, R_ref=ref)
    if not with_tau:
        return S
    v = np.r_[g.phi(), -1.0]
    d_r2 = lib.DeviceArray((g.nblocks,))
    lib.block_rows_residuals(d_tri, off, nc, lib.DeviceArray.from_host(v), d_r2)
    r2 = d_r2.to_host()
    for b in range(g.nblocks):
        if off[b + 1] == off[b]:
            assert r2[b] == 0.0
            continue
        sl = slice(b * g.rows_b, (b + 1) * g.rows_b)
        e2 = float(g.e[sl] @ g.e[sl])  # exact: integers
        c = qg.residual_ratio(r2[b], e2, v[np.r_[g.lists[b], n]], g.block_gram(b))
        worst_r2 = max(worst_r2, c)
        assert c <= C_R2, "%s: block %d residual %.17g, exact %.17g (%.3g u)" % (tag, b, r2[b], e2, c)
    record_property(tag + ":residual_over_u", "%.3e" % worst_r2)
    e2s = [float(g.e[sl] @ g.e[sl]) for sl in (slice(b * g.rows_b, (b + 1) * g.rows_b) for b in g.active())]
    assert max(e2s) / min(e2s) >= 2.0 ** 30
    return S


@pytest.mark.parametrize("profile", sorted(PROFILES))
@pytest.mark.parametrize("case", BLOCK_CASES, ids=[c[0] for c in BLOCK_CASES])
def test_blocks_graded_full_rank(lib, case, profile, record_property):
    """figh_tsqr_selected_blocks on full-rank graded row blocks, dense and block-compact W, with and without d_block_tri:
    the merged triangle (tol_qr < 0) against the exact Gram of the active rows with all three metrics, every block's rows
    of the stack against its own exact Gram, the per-block residuals against ||e_b||^2, and the pipeline's weighted TSQR
    over the stack (one power-of-two weight per row) against the exact row-weighted Gram."""
    name, spec, rows_b, with_tau = case
    g = _row_blocks(spec, rows_b, profile, False, [rows_b, len(profile), 3, len(name)])
    n = g.n
    nc = n + (1 if with_tau else 0)
    G = g.gram(with_tau)
    R_ref = qg.cholesky_ld(G)
    for compact in (False, True):
        for want_tri in (True, False):
            tag = "blocks_%s_%s%s" % (name, "compact" if compact else "dense", "_tri" if want_tri else "")
            R, d_tri = _run_blocks(lib, g, compact, with_tau, -1.0, want_tri)
            _check(np.triu(R), G, record_property, tag, R_ref=R_ref)
            if not want_tri:
                continue
            _check_stack(lib, g, d_tri, with_tau, False, record_property, tag)
            if not with_tau or compact:
                continue
            # the weighted solve of pipeline._wls: figh_tsqr over the stack rows, base columns + tau, one weight per row
            off = g.stack_offsets(with_tau)
            rng = np.random.default_rng(len(name))
            w = rng.integers(-3, 4, g.nblocks)
            row_w = np.repeat(np.ldexp(1.0, w), np.diff(off))
            cols = np.r_[np.arange(n), n].astype(np.int32)
            d_Rw = lib.DeviceArray((nc * nc,))
            lib.tsqr(d_tri, int(off[-1]), nc, lib.DeviceArray.from_host(cols), nc, None, row_w, d_Rw)
            Gw = g.gram(with_tau, cols=cols, block_exp=w)
            _check(np.triu(d_Rw.to_host().reshape(nc, nc)), Gw, record_property, tag + "_weighted")


@pytest.mark.parametrize("profile", sorted(PROFILES))
@pytest.mark.parametrize("case", BLOCK_CASES[:2], ids=[c[0] for c in BLOCK_CASES[:2]])
def test_blocks_graded_exact_dependencies(lib, case, profile, record_property):
    """The same entry with exact dependencies inside every column group: backward for the plain triangle and the stack,
    then tol_qr = 1e-8 -- exact base set, zero dependent rows, R1, the base rows and the residual; nc > 80 runs
    reveal_triangle's scatter, nc <= 80 the regrouping inside tsqr_reduce_stack."""
    name, spec, rows_b, with_tau = case
    g = _row_blocks(spec, rows_b, profile, True, [rows_b, len(profile), 5, len(name)])
    assert len(g.dep) > 10
    n = g.n
    G = np.asarray(g.gram(with_tau), dtype=np.float64)  # (exact: every entry is a sum of a few exact block entries)
    base = [k for k in g.base if k < n]
    for compact in (False, True):
        tag = "blocks_deps_%s_%s" % (name, "compact" if compact else "dense")
        R, d_tri = _run_blocks(lib, g, compact, with_tau, -1.0, True)
        _check(np.triu(R), g.gram(with_tau), record_property, tag, forward=False)
        _check_stack(lib, g, d_tri, with_tau, True, record_property, tag)
        rows_k, _ = _run_blocks(lib, g, compact, with_tau, TOL_QR, False)
        _check_regrouped(rows_k, G, n, with_tau, base, g.dep, record_property, tag, R_plain=R)


# ---------------------------------------------------------------------------------------------------- null-pivot rule
_null_bound, _null_rule_check = qg.null_bound, qg.null_rule_check  # (shared with test_streamed_columnwise.py)


@pytest.mark.parametrize("case", ["human", "talos"])
def test_null_pivot_rule_wrench_column_bound(lib, case, record_property):
    """The column bound of test_qr_graded.test_null_pivot_rule_graded_column_bound for the wrench entry (pieces = 6, as
    the pipeline passes them), force-compact and link-padded; the base set is the exact one with the rule on and off."""
    from figaroh_plus_amd import _lib
    c = {x[0]: x for x in WRENCH_CASES}[case]
    _, Nb, nlinks, n, dead, extra, with_tau, profile = c
    rng = np.random.default_rng([Nb, n, 17])
    g = qg.Wrench(rng, Nb, nlinks, n, *PROFILES[profile], dead_links=dead, extra_slots=extra, deps=True)
    G = g.gram(with_tau)
    base = [k for k in g.base if k < n]
    for layout in ("link-padded", "force-link-compact"):
        for rule in (False, True):
            with _lib.null_pivots(TOL_QR if rule else 0.0):
                R = _run_wrench(lib, g, layout, with_tau, -1.0)
            _null_rule_check(R, G, g.rows, 6, base, n, "null_wrench_%s_%s_%d" % (case, layout, rule), record_property, rule)


@pytest.mark.parametrize("case", ["wide", "narrow"])
def test_null_pivot_rule_blocks_column_bound(lib, case, record_property):
    """The same for the row-block entry (pieces = nblocks, as the pipeline passes them), dense and block-compact."""
    from figaroh_plus_amd import _lib
    name, spec, rows_b, with_tau = {x[0]: x for x in BLOCK_CASES}[case]
    g = _row_blocks(spec, rows_b, "wide", True, [rows_b, 23, len(name)])
    n = g.n
    G = g.gram(with_tau)
    base = [k for k in g.base if k < n]
    for compact in (False, True):
        for rule in (False, True):
            with _lib.null_pivots(TOL_QR if rule else 0.0):
                R, _ = _run_blocks(lib, g, compact, with_tau, -1.0, False)
            _null_rule_check(R, G, g.rows, g.nblocks, base, n,
                             "null_blocks_%s_%s_%d" % (case, "compact" if compact else "dense", rule), record_property, rule)


# ---------------------------------------------------------------------------------------------------- batched excitation TSQR
def _gram_ld(A):
    Al = np.asarray(A, dtype=np.longdouble)
    return Al.T @ Al


def _check_gram(R, G, record_property, tag):
    """Backward metric of a kernel-built W's triangle against a long-double Gram (test_qr_graded._check_against_W)."""
    assert np.array_equal(R, np.triu(R))
    b = qg.backward_err(R, G)
    record_property(tag + ":backward", "%.3e" % b)
    assert b <= TOL_BACKWARD, "%s: backward %.3e > %.1e" % (tag, b, TOL_BACKWARD)


# wide-kernel tile height of figh_regressor_tsqr_batch, 16 nrc of wy_config (figh_tsqr_wide_kernel.h) for these column counts
_BATCH_TILE = {179: 96, 234: 80, 164: 96}
# (cfg, B, n_per, stacked): UR10 / TX40 (r <= 80): one launch pair per trajectory.  TIAGo (r 179, 24 rows per sample),
# TALOS (234, 6), human (164, 6): the batched wide kernel -- wgs 16 (human), the 1024 / B cap (wgs 2 for B = 400, wgs 1 for
# B = 600) -- and TALOS with 6 n_per < 8 r: trajectory by trajectory with a wide r.  Every n_per is odd: never a multiple
# of the tile height.
BATCH_CASES = [("cfg2_ur10", 3, 1001, True), ("cfg1_tx40", 2, 517, False), ("cfg5_human", 3, 2011, True),
               ("cfg3_tiago", 400, 155, True), ("cfg4_talos", 600, 313, False), ("cfg4_talos", 2, 301, True)]


def _batch_wgs(r, rps, B, n_per):
    """Workgroups per trajectory the entry launches (figh_stream.hip), 0 for the trajectory-by-trajectory path."""
    if r <= 80 or rps * n_per < 8 * r:
        return 0
    M = _BATCH_TILE[r]
    cap = min(rps * (-(-n_per // M)) // 4, rps * n_per // (4 * r), max(1, 1024 // B))
    w = 1
    while 2 * w <= cap:
        w *= 2
    return w


def test_batch_cases_reach_every_path():
    """The (B, n_per) choices cover wgs = 1, wgs >= 4, the 1024 / B cap and the short-trajectory fall-back for a wide r."""
    shapes = {"cfg3_tiago": (179, 24), "cfg4_talos": (234, 6), "cfg5_human": (164, 6), "cfg2_ur10": (36, 6),
              "cfg1_tx40": (61, 6)}
    got = {(c, B, n): _batch_wgs(*shapes[c], B, n) for c, B, n, _ in BATCH_CASES}
    assert got[("cfg5_human", 3, 2011)] >= 4 and got[("cfg4_talos", 600, 313)] == 1
    assert got[("cfg3_tiago", 400, 155)] == 2 == 1024 // 400  # (the cap binds)
    assert got[("cfg4_talos", 2, 301)] == 0 and 234 > 80


@pytest.mark.parametrize("cfg,B,n_per,stacked", BATCH_CASES)
def test_regressor_tsqr_batch_columnwise(lib, cfg, B, n_per, stacked, record_property):
    """figh_regressor_tsqr_batch (excitation.base_regressor_triangles_batch) against the long-double Gram of the W that
    build_regressor_basic writes for trajectory b's samples, R_stack^T R_stack added when stacked.  For B in the hundreds a
    first, middle and last trajectory are checked (the Gram in long double is the cost)."""
    from conftest import Golden
    from figaroh_plus_amd.tools.excitation import base_columns, base_regressor_triangle, base_regressor_triangles_batch
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    from figaroh_plus_amd.tools.regressor import add_coupling_TX40, build_regressor_basic, regressor_flags
    g = Golden(cfg)
    robot = g.robot()
    rng = np.random.default_rng([B, n_per])
    trajs = [sample_inputs(robot.model, n_per, rng, 1.5, 2, 5) for _ in range(B)]
    mode, flags, _ = regressor_flags(g.param, g.coupling)
    rps, ncols = robot.device_model().shape(mode, flags)
    cols = base_columns(ncols, g["idx_e"], g["idx_base"])
    r = len(cols)
    wgs = _batch_wgs(r, rps, B, n_per)
    record_property("batch_wgs", str(wgs))
    G0 = np.zeros((r, r), dtype=np.longdouble)
    R_stack = None
    if stacked:
        qs, vs, as_ = sample_inputs(robot.model, 200, rng, 1.5, 2, 5)
        R_stack = base_regressor_triangle(robot, qs, vs, as_, g.param, g["idx_e"], g["idx_base"], coupling=g.coupling)
        G0 = _gram_ld(np.triu(R_stack))
    R = base_regressor_triangles_batch(robot, trajs, g.param, g["idx_e"], g["idx_base"], R_stack=R_stack, coupling=g.coupling)
    assert R.shape == (B, r, r)
    for b in sorted({0, B // 2, B - 1}):
        q, v, a = trajs[b]
        W = build_regressor_basic(robot, q, v, a, dict(g.param))
        if g.coupling:
            m = robot.model
            W = add_coupling_TX40(W, m, robot.data, n_per, m.nq, m.nv, m.njoints, q, v, a)
        assert W.shape == (rps * n_per, ncols)
        _check_gram(R[b], G0 + _gram_ld(W[:, cols]), record_property, "batch_%s_wgs%d" % (cfg, wgs))


# ---------------------------------------------------------------------------------------------------- the pipeline's own W
def _pipeline(cfg, N, w_layout, seed):
    from conftest import Golden
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    g = Golden(cfg)
    robot = g.robot()
    q, v, a = sample_inputs(robot.model, N, np.random.default_rng(seed), 1.5, 2, 5)
    pipe = IdentificationPipeline(robot, g.param, params_std=g.params_std(), coupling=g.coupling, w_layout=w_layout)
    pipe.set_samples(q, v, a)
    pipe.set_tau_from_parameters(g.phi_ref(), noise_std=0.05, seed=3)
    pipe.run()
    return g, robot, pipe, (q, v, a)


def _pipeline_inputs(lib, pipe, W_ref):
    """Kept columns (reference numbering), host tau and the column norms of the pass (the pipeline's device copy)."""
    ncols = W_ref.shape[1]
    tau = pipe.d_tau.to_host()[:W_ref.shape[0]]
    cs = pipe._d_pack.to_host()[:ncols]
    kept = np.flatnonzero(~(cs < pipe.tol_e))
    assert np.array_equal(kept, np.flatnonzero(pipe._mask_expected))
    return kept, tau, cs


# (the pipeline takes the force-compact layout only when 3 N >= 16 (ncols + 1): TALOS 462, human 560 reference columns)
@pytest.mark.parametrize("cfg,N", [("cfg4_talos", 2500 + 5), ("cfg5_human", 3000 + 5)])
def test_pipeline_wrench_W_through_the_entry(lib, cfg, N, record_property):
    """The force-compact W an IdentificationPipeline pass wrote (TALOS: link-padded torque rows; human: link-compact) read
    back through the layout maps equals the reference-layout W of build_regressor_basic -- the maps confirmed against the
    regressor kernels -- and figh_tsqr_selected_wrench on that buffer (tol_qr < 0) against the long-double Gram of it."""
    from figaroh_plus_amd.tools.regressor import build_regressor_basic
    g, robot, pipe, (q, v, a) = _pipeline(cfg, N, "dense", 11)
    W = pipe.W
    assert getattr(W, "force_ld", 0) > 0 and (cfg == "cfg4_talos") == (pipe._link_pos is None)
    ncols = W.ref_cols
    back = qg.read_wrench_layout(W.buf.to_host(), W.rows, ncols, W.ld, 16, pipe._link_pos, W.force_ld)
    W_ref = build_regressor_basic(robot, q, v, a, dict(g.param))
    scale = np.abs(W_ref).max(axis=0)
    assert (np.abs(back - W_ref) <= 1e-12 * np.where(scale > 0, scale, 1.0)).all(), "layout maps disagree with the regressor"
    kept, tau, cs = _pipeline_inputs(lib, pipe, back)
    n = len(kept)
    nf = int(np.count_nonzero(kept % 14 >= 6))
    assert 3 * N >= 16 * (n + 1) and n + 1 > 80
    d_sel = lib.DeviceArray((2 + 2 * ncols,), np.int32)
    d_R = lib.DeviceArray(((n + 2) * (n + 1),))
    lib.tsqr_selected_wrench(W.buf, W.rows, W.ld, lib.DeviceArray.from_host(cs), ncols, pipe.tol_e, 16, n, nf,
                             lib.DeviceArray.from_host(tau), -1.0, d_sel, d_R, d_link_pos=pipe._d_link_pos,
                             ld_force=W.force_ld)
    assert d_sel.to_host()[0] == n
    R = np.triu(d_R.to_host()[:(n + 1) ** 2].reshape(n + 1, n + 1))
    _check_gram(R, _gram_ld(np.c_[back[:, kept], tau]), record_property, "pipeline_wrench_%s" % cfg)


@pytest.mark.parametrize("w_layout", ["dense", "block-compact"])
def test_pipeline_tiago_W_through_the_blocks_entry(lib, w_layout, record_property):
    """TIAGo's W (link-padded or block-compact) from an IdentificationPipeline pass at N = 4096 + 37 -- the grouped launches
    run with the real column lists -- read back block by block equals build_regressor_basic's W; figh_tsqr_selected_blocks
    on that buffer (tol_qr < 0, with d_block_tri): every block's rows of the stack against the long-double Gram of its
    [W_j[:, list_j] tau_j]."""
    from figaroh_plus_amd.tools.regressor import build_regressor_basic
    N = 4096 + 37
    g, robot, pipe, (q, v, a) = _pipeline("cfg3_tiago", N, w_layout, 12)
    W = pipe.W
    ncols = W.ref_cols
    nb = robot.model.nv
    W_ref = build_regressor_basic(robot, q, v, a, dict(g.param))
    buf = W.buf.to_host()
    c = np.arange(ncols)
    back = np.zeros_like(W_ref)
    compact = getattr(W, "compact", None)
    for j in range(nb):
        rows = slice(j * N, (j + 1) * N)
        if compact is None:
            Wj = buf[j * N * W.ld:(j + 1) * N * W.ld].reshape(N, W.ld)
            back[rows] = Wj[:, 16 * (c // 14) + c % 14]
        else:
            off, ld = int(compact[0][j]), int(compact[1][j])
            Wj = buf[off:off + N * ld].reshape(N, ld)
            win = (c // 14 >= j) & (c // 14 < j + ld // 16)  # the window of joint j's subtree
            back[rows][:, win] = Wj[:, 16 * (c[win] // 14 - j) + c[win] % 14]
    scale = np.abs(W_ref).max(axis=0)
    assert (np.abs(back - W_ref) <= 1e-12 * np.where(scale > 0, scale, 1.0)).all(), "layout disagrees with the regressor"
    kept, tau, cs = _pipeline_inputs(lib, pipe, back)
    n = len(kept)
    nc = n + 1
    blocks = pipe._block_lists(ncols, 16)
    counts = np.asarray(blocks[1])
    assert (counts >= 1).sum() >= 4 and n == int(pipe._n_expected)
    d_sel = lib.DeviceArray((2 + 2 * ncols,), np.int32)
    d_R = lib.DeviceArray(((nc + 1) * nc,))
    d_tri = lib.DeviceArray(((int((counts + 1).sum()) + nc + 1) * nc,))
    off = ld = None
    if compact is not None:
        off, ld = compact
    lib.tsqr_selected_blocks(W.buf, W.rows, W.ld, lib.DeviceArray.from_host(cs), ncols, pipe.tol_e, 16, n, counts,
                             blocks[4] if compact is not None else blocks[2], blocks[3], lib.DeviceArray.from_host(tau),
                             -1.0, d_sel, d_R, block_off=off, block_ld=ld, d_block_tri=d_tri)
    assert d_sel.to_host()[0] == n
    S = d_tri.to_host()
    pos_all = blocks[3].to_host()
    at = row = 0
    for j in range(nb):
        L = np.asarray(pos_all[at:at + counts[j]], dtype=np.int64)
        at += counts[j]
        Sj = S[row * nc:(row + counts[j] + 1) * nc].reshape(counts[j] + 1, nc)
        row += counts[j] + 1
        cols = np.r_[L, n]
        assert not np.delete(Sj, cols, axis=1).any()
        rows = slice(j * N, (j + 1) * N)
        _check_gram(np.triu(Sj[:, cols]), _gram_ld(np.c_[back[rows][:, kept[L]], tau[rows]]), record_property,
                    "pipeline_tiago_%s_b%d" % (w_layout, j))
