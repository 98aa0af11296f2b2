"""GPU suite: column norms, residual sums and normal-equation terms column by column (and joint by joint).

The QR checks moved to column-wise metrics (test_qr_graded.py, test_qr_structured_graded.py); the reductions upstream of
the QR decide which columns reach it (``col_norm[i] < tol_e``, an absolute threshold, regressor.py:271) and with what
weight (1 / sigma_j).  The older checks of test_gpu_parity.py divide by the largest column norm, which cannot tell a norm
of 0 from one of 5e-6 next to tol_e = 1e-6.  Here:

1. exact input -- integer entries with power-of-two scales, every partial sum exact in any order: figh_colsq,
   figh_matvec, figh_block_sqnorm must be bit-exact;
2. the norms of a kernel-built W against long-double sums of the W that kernel wrote, per column within the a-priori
   gamma_m (tests/reductions_common.py) -- K1 (chain), K1' (tree: fused norms and the figh_colsq fallback, the random
   trees of test_gpu_parity._TREES), the fused chain pass, the norms-only entries and the pipeline's passes;
3. the elimination decision at tol_e: copied columns (Ia, fv, the TX40 coupling columns) at tol_e (1 +- 1e-9), computed
   inertia-tensor columns at tol_e (1 +- 1e-6), a prefix that crosses, shards that cross only in their sum
   (tools/fuzz_sharded.ReplayExchange) and a tol_e sweep: the exact split in the paths each case names;
4. figh_regressor_gram entry by entry, and sigma2_joint joint by joint from both WLS sources.

Measured ratios are recorded as test properties (``--junitxml``).  The module takes about 30 s on an MI355X (28.8 s of
test time measured).
"""
import numpy as np
import pytest

import qr_graded_common as qg
import reductions_common as rc
from qr_graded_common import TOL_BACKWARD

pytestmark = pytest.mark.gpu

# figh_regressor_colsq / figh_regressor_tsqr_norms never store W: their reference is the W figh_regressor_build writes for
# the same samples.  Slack for the differences between the two kernels' W (relative, per column).  Measured on an MI355X:
# every such column within 3.6e-4 of gamma_m + SIBLING_SLACK, i.e. inside gamma_m alone (the W are the same)
SIBLING_SLACK = 1e-13
# Largest ratios measured on an MI355X (the bounds themselves are a-priori): K1 chain 0.65 gamma_m (6 rows, N = 1), K1'
# tree 8.7e-3, pipeline passes 1.3e-4, random trees 1.2e-4, figh_regressor_gram 3.2e-2 TOL_BACKWARD, sigma2 direct 1.7e-4
# of its bound, sigma2 per-row-block triangles 2.1e-3 of the tight bound.
TOL_E = 1e-6


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    qg.check_longdouble()
    return _lib


def _pow2(s):
    return np.ldexp(1.0, np.asarray(s, dtype=np.int64))


def _colsq_ok(cs, ref, m, tag, record_property, slack=0.0):
    """Per column: |cs_j - cs*_j| / cs*_j <= gamma_m + slack, cs_j == 0 where cs*_j == 0; records both ratios."""
    r = rc.colsq_ratio(cs, ref, m, slack)
    record_property(tag + ":over_bound", "%.3e" % float(np.max(r, initial=0.0)))
    record_property(tag + ":over_log2m_u", "%.3e" % rc.colsq_worst_over_log_u(cs, ref, m))
    bad = np.flatnonzero(~(r <= 1.0))
    assert bad.size == 0, "%s: columns %s off their reference (%s vs %s, bound %.3g)" % (
        tag, bad[:8].tolist(), np.asarray(cs)[bad[:4]], np.asarray(ref, dtype=np.float64)[bad[:4]], rc.gamma(m) + slack)


def _ld_colsq_device(d_W, rows, ld, cols, chunk=rc.ROW_CHUNK):
    """Long-double column sums of squares of a rows x ld device matrix (first ``cols`` columns), read back in row chunks."""
    from figaroh_plus_amd import _lib
    out = np.zeros(cols, dtype=np.longdouble)
    host = np.empty(max(1, min(rows, chunk) * ld))
    for r0 in range(0, rows, chunk):
        nr = min(chunk, rows - r0)
        h = host[:nr * ld]
        _lib.check(_lib.load().figh_memcpy_d2h(h.ctypes.data, d_W.ptr + 8 * r0 * ld, h.nbytes))
        X = np.asarray(h.reshape(nr, ld)[:, :cols], dtype=np.longdouble)
        out += (X * X).sum(axis=0)
    return out


# ---------------------------------------------------------------------------------------------------- 1. exact input
def _colsq_rows(lib, key):
    """The rows_per_block edges of figh_colsq: cu_count * 8 blocks of at least 16 rows."""
    if isinstance(key, int):
        return key
    edge = lib.device_info()["cu_count"] * 8 * 16
    return edge + {"edge-1": -1, "edge": 0, "edge+1": 1}[key]


COLSQ_COLS = [1, 14, 84, 87, 255, 256, 257, 560, 1024]


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 255, 257, "edge-1", "edge", "edge+1", 20011, 1000003])
def test_colsq_exact(lib, rows):
    """figh_colsq on integer W with column scales 2^-30 .. 2^30, all-zero columns, a column whose only non-zero entry is
    in the last row, ldw > cols with NaN in the padding: equal to diag of the exact Gram, bit for bit."""
    rows = _colsq_rows(lib, rows)
    for cols in ([84, 87] if rows > 10 ** 6 else COLSQ_COLS):
        rng = np.random.default_rng([rows, cols])
        M = qg.int_matrix(rng, rows, cols)
        s = rng.integers(-30, 31, cols)
        if cols >= 3:
            M[:, rng.choice(cols, max(1, cols // 9), replace=False)] = 0.0
            j = int(rng.integers(cols))
            M[:, j] = 0.0
            M[-1, j] = 1000.0
        ldw = cols + 3
        W = np.full((rows, ldw), np.nan)
        W[:, :cols] = M * _pow2(s)
        d_W = lib.DeviceArray.from_host(W.reshape(-1))
        del W
        d_out = lib.DeviceArray((cols,))
        lib.colsq(d_W, rows, cols, ldw, d_out)
        got = d_out.to_host()
        ref = rc.exact_colsq(M, s)
        assert np.array_equal(got, ref), "rows %d cols %d: %d columns differ" % (rows, cols, int((got != ref).sum()))


@pytest.mark.parametrize("rows", [0, 1, 3, 4, 5, 63, 64, 65, 20011])
def test_matvec_exact(lib, rows):
    """figh_matvec on integer W and x with power-of-two ROW scales (every y_r exact), the first n columns of a wider W
    (NaN behind them) and a gathered list (out of order, a repeated index): bit-exact; rows = 0 writes nothing."""
    for n in [1, 63, 64, 65, 129, 560]:
        for gathered in (False, True):
            rng = np.random.default_rng([rows, n, int(gathered)])
            ldw = n + (37 if gathered else 5)
            M = qg.int_matrix(rng, rows, ldw)
            e = rng.integers(-30, 31, rows)
            W = M * _pow2(e)[:, None]
            x = qg.int_matrix(rng, 1, n)[0]
            if gathered:
                idx = rng.integers(0, ldw, n).astype(np.int32)
                if n > 2:
                    idx[1] = idx[n - 1]
                d_idx = lib.DeviceArray.from_host(idx)
            else:
                idx = np.arange(n)
                W[:, n:] = np.nan
                d_idx = None
            y0 = np.full(max(rows, 1), 7.0)
            d_y = lib.DeviceArray.from_host(y0)
            lib.matvec(lib.DeviceArray.from_host(W.reshape(-1) if rows else np.zeros(1)), rows, ldw, d_idx, n,
                       lib.DeviceArray.from_host(x), d_y)
            y = d_y.to_host()
            if rows == 0:
                assert np.array_equal(y, y0), "rows = 0 wrote to y"
                continue
            ref = (M[:, idx].astype(np.int64) @ x.astype(np.int64)).astype(np.float64) * _pow2(e)
            assert np.array_equal(y, ref), "rows %d n %d gathered %s: %d rows differ" % (
                rows, n, gathered, int((y != ref).sum()))


def _block_sq_ref(a_int, b_int, e, lens):
    out, off = [], 0
    for k, n in enumerate(lens):
        d = a_int[off:off + n] - (b_int[off:off + n] if b_int is not None else 0)
        out.append(float(int((d * d).sum())) * 4.0 ** float(e[k]))
        off += n
    return np.array(out)


@pytest.mark.parametrize("nblocks", [1, 2, 6, 7, 12])
def test_block_sqnorm_exact(lib, nblocks):
    """figh_block_sqnorm on integer a, b (a - b exact) with per-block scales from 2^-40 to 2^40 -- one block's sum 2^160
    times another's -- with and without b: bit-exact."""
    for rb in [1, 255, 256, 257, 4097]:
        rng = np.random.default_rng([nblocks, rb])
        e = rng.permutation(np.linspace(-40, 40, nblocks).round().astype(np.int64)) if nblocks > 1 else np.array([40])
        rows = nblocks * rb
        ai = rng.integers(-1024, 1025, rows)
        bi = rng.integers(-1024, 1025, rows)
        sc = np.repeat(_pow2(e), rb)
        d_out = lib.DeviceArray((nblocks,))
        d_a = lib.DeviceArray.from_host(ai * sc)
        for with_b in (True, False):
            lib.block_sqnorm(d_a, lib.DeviceArray.from_host(bi * sc) if with_b else None, rows, nblocks, d_out)
            ref = _block_sq_ref(ai, bi if with_b else None, e, [rb] * nblocks)
            assert np.array_equal(d_out.to_host(), ref), "nblocks %d rows/block %d b %s" % (nblocks, rb, with_b)


def test_block_residual_sqnorms_list_path(lib):
    """identification_tools.block_residual_sqnorms with unequal block lengths (one launch per block, blocks of length 1):
    bit-exact against the integer sums."""
    from figaroh_plus_amd.identification.identification_tools import block_residual_sqnorms
    rng = np.random.default_rng(5)
    lens = [1, 257, 4097, 3, 1, 1000]
    e = np.array([-40, 40, 0, -17, 23, 5])
    rows = sum(lens)
    ai, bi = rng.integers(-1024, 1025, rows), rng.integers(-1024, 1025, rows)
    sc = np.repeat(_pow2(e), lens)
    got = block_residual_sqnorms(ai * sc, bi * sc, lens)
    assert np.array_equal(got, _block_sq_ref(ai, bi, e, lens))


# ---------------------------------------------------------------------------------------------------- 2. kernel-built norms
def _robot(name):
    """(robot, coupling, Golden or None): a golden config, or a synthetic serial chain 'chainK'."""
    from conftest import Golden
    if name.startswith("cfg"):
        g = Golden(name)
        return g.robot(), g.coupling, g
    from test_gpu_parity import _synthetic_chain
    return _synthetic_chain(int(name[5:])), False, None


def _param(fl, wrench=False):
    return dict(is_joint_torques=not wrench, is_external_wrench=wrench, has_friction=bool(fl & 1),
                has_actuator_inertia=bool(fl & 2), has_joint_offset=bool(fl & 4), force_torque=["All"] if wrench else None)


def _inputs(robot, N, seed, kind, golden=None):
    """(q, v, a): the golden samples (cycled to N), uniform samples, or inputs with a wide column spread -- one joint
    nearly at rest ("rest"), small v and a on the two distal joints ("distal")."""
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    m = robot.model
    if kind == "golden" and golden is not None:
        idx = np.arange(N) % golden["q_big"].shape[0]
        return golden["q_big"][idx].copy(), golden["v_big"][idx].copy(), golden["a_big"][idx].copy()
    rng = np.random.default_rng(seed)
    q, v, a = sample_inputs(m, N, rng, 1.5, 2, 5)
    if kind == "rest":
        j = int(rng.integers(m.nv))
        v[:, j] *= 1e-5
        a[:, j] *= 1e-5
    elif kind == "distal":
        v[:, -2:] *= 1e-3
        a[:, -2:] *= 1e-3
    return q, v, a


def _k1(lib, robot, param, coupling, q, v, a, extra_flags=0, ldw_extra=0):
    """figh_regressor_build with d_colsq: (d_W, ldw, ncols, rows, colsq)."""
    from figaroh_plus_amd.tools.regressor import _samples_to_device, regressor_flags
    mode, flags, ft = regressor_flags(param, coupling)
    flags |= extra_flags
    h = robot.device_model()
    rps, ncols = h.shape(mode, flags)
    N, d_q, d_v, d_a = _samples_to_device(robot.model, q, v, a)
    ldw = ncols + ldw_extra
    d_W = lib.DeviceArray((max(1, rps * N * ldw),))
    d_cs = lib.DeviceArray((ncols,))
    lib.regressor_build(h, mode, flags, ft, N, d_q, d_v, d_a, d_W, ldw, d_cs)
    return d_W, ldw, ncols, rps * N, d_cs.to_host()


CHAIN_MODELS = ["cfg1_tx40", "cfg2_ur10", "chain5", "chain6", "chain7"]


@pytest.mark.parametrize("fl", range(8))
@pytest.mark.parametrize("model", CHAIN_MODELS)
def test_k1_chain_colsq_against_its_W(lib, model, fl, record_property):
    """The chain regressor kernel's fused norms against the long-double sums of the W it wrote, per column within gamma_m,
    zero columns exactly zero: TX40 with its coupling columns, UR10, 5/6/7-link chains, all eight flag combinations, N from
    1 to 20011, golden inputs and inputs with a wide column spread."""
    robot, coupling, g = _robot(model)
    param = _param(fl)
    for N in [1, 63, 64, 65, 4097, 20011]:
        kinds = ["golden", "rest", "distal"] if N <= 65 else (["rest"] if N == 4097 else ["distal"])
        for kind in kinds:
            q, v, a = _inputs(robot, N, [N, fl, len(model)], kind, g)
            d_W, ldw, ncols, rows, cs = _k1(lib, robot, param, coupling, q, v, a)
            ref = _ld_colsq_device(d_W, rows, ldw, ncols)
            _colsq_ok(cs, ref, rows, "k1_%s_f%d_N%d_%s" % (model, fl, N, kind), record_property)


def test_k1_chain_colsq_million_samples(lib, record_property):
    """UR10 at 10^6 samples (the grid-stride tile loop of the chain kernel), actuator inertia and friction on."""
    robot, coupling, g = _robot("cfg2_ur10")
    q, v, a = _inputs(robot, 1000000 + 3, 77, "distal")
    d_W, ldw, ncols, rows, cs = _k1(lib, robot, _param(3), coupling, q, v, a)
    ref = _ld_colsq_device(d_W, rows, ldw, ncols)
    _colsq_ok(cs, ref, rows, "k1_ur10_1e6", record_property)


# (cfg, extra flags, ldw - ncols): the tree kernel's fused norms need an even column count, an even ldw and an aligned W;
# otherwise figh_regressor_build runs figh_colsq on what it wrote (colsq_done = 0)
K1_TREE_CASES = {"tx40_generic_87": ("cfg1_tx40", 256, 0), "ur10_generic_odd_ldw": ("cfg2_ur10", 256, 1),
                 "tiago_odd_ldw": ("cfg3_tiago", 0, 1), "tiago": ("cfg3_tiago", 0, 0), "talos": ("cfg4_talos", 0, 0),
                 "human": ("cfg5_human", 0, 0)}


@pytest.mark.parametrize("case", sorted(K1_TREE_CASES))
def test_k1_tree_colsq_and_fallback(lib, case, record_property):
    """figh_regressor_build through the tree kernel (reference layout): the fused norms on an aligned even-width W, and the
    figh_colsq fallback for an odd column count (TX40, 87 columns, force_generic_kernel) or an odd ldw."""
    from conftest import Golden
    cfg, extra, ldw_extra = K1_TREE_CASES[case]
    g = Golden(cfg)
    robot = g.robot()
    for N in [63, 1025]:
        q, v, a = _inputs(robot, N, [N, 3], "rest")
        d_W, ldw, ncols, rows, cs = _k1(lib, robot, dict(g.param), g.coupling, q, v, a, extra_flags=extra,
                                        ldw_extra=ldw_extra)
        ref = _ld_colsq_device(d_W, rows, ldw, ncols)
        _colsq_ok(cs, ref, rows, "k1tree_%s_N%d" % (case, N), record_property)


@pytest.mark.parametrize("cfg", ["cfg2_ur10", "cfg1_tx40", "cfg3_tiago", "cfg5_human"])
def test_norms_only_entries(lib, cfg, record_property):
    """figh_regressor_colsq and figh_regressor_tsqr_norms (chunk partials + vec_add_kernel, or the tree kernel's
    accumulation) with chunk_samples 0, 64, 150 and N - 1 (a ragged last chunk), against the long-double sums of the W
    figh_regressor_build writes for the same samples, within gamma_m + SIBLING_SLACK."""
    from conftest import Golden
    from figaroh_plus_amd.tools.regressor import _samples_to_device, regressor_flags
    g = Golden(cfg)
    robot = g.robot()
    N = 1537
    q, v, a = _inputs(robot, N, 9, "distal")
    d_W, ldw, ncols, rows, _ = _k1(lib, robot, g.param, g.coupling, q, v, a)
    ref = _ld_colsq_device(d_W, rows, ldw, ncols)
    d_W.free()
    mode, flags, ft = regressor_flags(g.param, g.coupling)
    h = robot.device_model()
    _, d_q, d_v, d_a = _samples_to_device(robot.model, q, v, a)
    kept = np.flatnonzero(np.asarray(ref, dtype=np.float64) >= TOL_E).astype(np.int32)
    n = len(kept)
    d_idx = lib.DeviceArray.from_host(kept)
    d_R = lib.DeviceArray((n * n,))
    for chunk in [0, 64, 150, N - 1]:
        d_cs = lib.DeviceArray((ncols,))
        lib.regressor_colsq(h, mode, flags, ft, N, d_q, d_v, d_a, d_cs, chunk_samples=chunk)
        _colsq_ok(d_cs.to_host(), ref, rows, "colsq_only_%s_c%d" % (cfg, chunk), record_property, SIBLING_SLACK)
        d_cs2 = lib.DeviceArray((ncols,))
        lib.regressor_tsqr(h, mode, flags, ft, N, d_q, d_v, d_a, d_idx, n, None, None, d_R, chunk_samples=chunk,
                           d_colsq=d_cs2)
        _colsq_ok(d_cs2.to_host(), ref, rows, "tsqr_norms_%s_c%d" % (cfg, chunk), record_property, SIBLING_SLACK)


# ---------------------------------------------------------------------------------------------------- the pipeline's passes
def _read_tree(pipe, N, ncols):
    """The resident joint-torque W of a tree of single-dof joints (TIAGo, the _TREES models; link-padded or block-compact,
    depth-first numbering) in the reference layout."""
    W = pipe.W
    buf = W.buf.to_host()
    nb = pipe.robot.model.nv
    c = np.arange(ncols)
    back = np.zeros((nb * N, ncols))
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
    return back


def _pipe_W(pipe, N):
    """The pass's own W in the reference layout (chains: the dense W; trees: the padded / compact layouts read back)."""
    W = pipe.W
    ncols = W.ref_cols
    if not pipe._padded:
        return W.buf.to_host()[:W.rows * W.ld].reshape(W.rows, W.ld)[:, :ncols]
    if pipe._flags()[0] == 0:  # joint torques of a tree
        return _read_tree(pipe, N, ncols)
    return qg.read_wrench_layout(W.buf.to_host(), W.rows, ncols, W.ld, 16, pipe._link_pos, getattr(W, "force_ld", 0))


def _pipeline(cfg, q, v, a, tau=None, param=None, **kw):
    """An IdentificationPipeline on (q, v, a); tau given, or W phi + noise (phi_ref for the golden param, ones otherwise)."""
    from conftest import Golden
    g = Golden(cfg)
    robot = g.robot()
    std = g.params_std() if param is None else robot.get_standard_parameters(param)
    phi = g.phi_ref() if param is None else None
    param = dict(g.param) if param is None else param
    return g, robot, _pipeline_of(robot, param, q, v, a, tau, std, phi, coupling=g.coupling, **kw)


def _pipeline_of(robot, param, q, v, a, tau=None, std=None, phi=None, **kw):
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    std = robot.get_standard_parameters(param) if std is None else std
    pipe = IdentificationPipeline(robot, param, params_std=std, **kw)
    pipe.set_samples(q, v, a, tau)
    if tau is None:
        pipe.set_tau_from_parameters(np.ones(len(pipe.names)) if phi is None else phi, noise_std=0.01, seed=1)
    return pipe


PIPE_CASES = [("cfg2_ur10", "dense", {}), ("cfg1_tx40", "dense", {}), ("cfg2_ur10", "dense", dict(fuse=False)),
              ("cfg3_tiago", "dense", {}), ("cfg3_tiago", "block-compact", {}), ("cfg4_talos", "dense", {}),
              ("cfg4_talos", "link-padded", {}), ("cfg4_talos", "link-compact", {}), ("cfg5_human", "dense", {}), ("cfg5_human", "link-compact", {}),
              ("cfg5_human", "link-padded", {})]


@pytest.mark.parametrize("cfg,layout,kw", PIPE_CASES,
                         ids=["%s-%s%s" % (c, l, "-nofuse" if k else "") for c, l, k in PIPE_CASES])
def test_pipeline_col_norm_against_its_W(lib, cfg, layout, kw, record_property):
    """out["col_norm"] of every pass kind against the long-double sums of the pass's own W: the chain's first pass
    (prefix + fused) and second pass (fused), fuse=False, TIAGo dense / block-compact (K1' fused norms), TALOS and the
    human model force-compact, link-padded and link-compact.  idx_e is the exact split."""
    from conftest import Golden
    N = 5003 if cfg in ("cfg2_ur10", "cfg1_tx40") else 3001
    q, v, a = _inputs(Golden(cfg).robot(), N, [N, len(layout)], "rest")
    g, robot, pipe = _pipeline(cfg, q, v, a, w_layout=layout, **kw)
    for p in range(2):
        out = pipe.run()
        back = _pipe_W(pipe, N)
        ref = rc.colsq_ld(back)
        _colsq_ok(out["col_norm"], ref, back.shape[0], "pipe_%s_%s_pass%d" % (cfg, layout, p), record_property)
        assert not rc.undecided(ref, pipe.tol_e, 1e-10)
        assert out["idx_e"] == rc.exact_split(ref, pipe.tol_e)[0]
    if cfg == "cfg2_ur10" and not kw:
        assert pipe.prefix_passes == 1 and pipe.fused_passes == 2


@pytest.mark.parametrize("cfg", ["cfg2_ur10", "cfg3_tiago"])
def test_pipeline_chunked_col_norm(lib, cfg, record_property):
    """A chunked pass keeps no W: its col_norm (figh_regressor_colsq, then figh_regressor_tsqr_norms) against the W of
    figh_regressor_build for the same samples, with the sibling slack."""
    from conftest import Golden
    g0 = Golden(cfg)
    N = 3001
    q, v, a = _inputs(g0.robot(), N, [N, 8], "distal")
    d_W, ldw, ncols, rows, _ = _k1(lib, g0.robot(), g0.param, g0.coupling, q, v, a)
    ref = _ld_colsq_device(d_W, rows, ldw, ncols)
    d_W.free()
    g, robot, pipe = _pipeline(cfg, q, v, a, chunk_samples=700)
    for p in range(2):
        out = pipe.run()
        _colsq_ok(out["col_norm"], ref, rows, "pipe_chunked_%s_pass%d" % (cfg, p), record_property, SIBLING_SLACK)
        assert out["idx_e"] == rc.exact_split(ref, pipe.tol_e)[0]


@pytest.mark.parametrize("shape", ["chain13", "binary15", "caterpillar", "star", "fork"])
def test_random_trees_colsq(lib, shape, record_property):
    """The random trees of test_gpu_parity._TREES (every shape the tree kernel's windowing distinguishes, a massless link in
    'fork'), friction / inertia / offset on, one joint nearly at rest: K1' in the reference layout (fused norms) and the
    pipeline's passes link-padded and block-compact, per column against the long-double norms of their own W; idx_e the
    exact split."""
    from test_gpu_parity import _TREES, _synthetic_tree
    parents = _TREES[shape]
    robot = _synthetic_tree(parents, seed=len(parents), massless=(4,) if shape == "fork" else ())
    param = _param(7)
    N = 64 * 20 + 17
    q, v, a = _inputs(robot, N, [N, len(parents)], "rest")
    d_W, ldw, ncols, rows, cs = _k1(lib, robot, param, False, q, v, a)
    _colsq_ok(cs, _ld_colsq_device(d_W, rows, ldw, ncols), rows, "tree_%s_k1" % shape, record_property)
    d_W.free()
    for layout in ("link-padded", "block-compact"):
        pipe = _pipeline_of(robot, param, q, v, a, w_layout=layout)
        for p in range(2):
            out = pipe.run()
            back = _pipe_W(pipe, N)
            ref = rc.colsq_ld(back)
            _colsq_ok(out["col_norm"], ref, rows, "tree_%s_%s_pass%d" % (shape, layout, p), record_property)
            assert not rc.undecided(ref, TOL_E, 1e-10)
            assert out["idx_e"] == rc.exact_split(ref, TOL_E)[0]


# ---------------------------------------------------------------------------------------------------- 3. the decision at tol_e
# UR10 with actuator inertia and friction: (joint, slot, side) of the copied columns put a hair off tol_e -- Ia_j (slot
# 10) is a_j, fv_j (slot 11) is v_j (oracle_np.build_regressor_basic)
UR10_STRADDLE = [(0, 10, -1), (2, 10, 1), (1, 11, 1), (3, 11, -1), (4, 10, 1), (5, 11, -1)]


def _straddle_ur10(N, seed, prefix=None):
    """UR10 inputs with the UR10_STRADDLE columns at tol_e (1 +- 1e-9).  ``prefix``: joint 2's Ia column at 0.5 tol_e over
    the first ``prefix`` samples, just above tol_e over all N.  Returns (q, v, a, {column: side})."""
    from conftest import Golden
    q, v, a = _inputs(Golden("cfg2_ur10").robot(), N, seed, "uniform")
    sides = {}
    for j, slot, side in UR10_STRADDLE:
        x = a if slot == 10 else v
        x[:, j], _ = rc.straddle(x[:, j], TOL_E, side)
        sides[14 * j + slot] = side
    if prefix is not None:
        a[:prefix, 2], _ = rc.scale_to_norm(a[:prefix, 2], 0.5 * TOL_E)
        a[prefix:, 2], _ = rc.scale_to_norm(a[prefix:, 2], 0.5 * TOL_E)
        a[:, 2] *= np.sqrt(float(TOL_E * (1 + 1e-9) / rc.colsq_ld(a[:, 2:3])[0]))
        assert rc.colsq_ld(a[:, 2:3])[0] > TOL_E * (1 + 0.99e-9) and rc.colsq_ld(a[:prefix, 2:3])[0] < TOL_E
    return q, v, a, sides


def _check_split(out_idx_e, ref, tag):
    idx_e, _ = rc.exact_split(ref, TOL_E)
    assert list(out_idx_e) == idx_e, "%s: split differs from the exact one at %s" % (
        tag, sorted(set(out_idx_e) ^ set(idx_e)))


def test_copied_columns_at_tol_e_chain(lib):
    """Six copied columns of UR10 at tol_e (1 +- 1e-9): the exact split in the drop-in get_index_eliminate /
    eliminate_non_dynaffect on the kernel's W, figh_tsqr_selected's d_sel, and the pipeline's first pass (prefix + fused),
    second pass (fused), fuse=False and chunk_samples."""
    from figaroh_plus_amd.tools.regressor import eliminate_non_dynaffect, get_index_eliminate
    N = 5003
    q, v, a, sides = _straddle_ur10(N, 31)
    param = _param(3)
    robot, coupling, _ = _robot("cfg2_ur10")
    d_W, ldw, ncols, rows, cs = _k1(lib, robot, param, coupling, q, v, a)
    W = d_W.to_host().reshape(rows, ldw)
    ref = rc.colsq_ld(W)
    for c, side in sides.items():  # the copied columns hold the scaled inputs
        assert (ref[c] > TOL_E) == (side > 0)
    assert not rc.undecided(ref, TOL_E, 1e-10)
    idx_e_ref, kept_ref = rc.exact_split(ref, TOL_E)
    names = list(robot.get_standard_parameters(param).keys())
    params_std = dict(zip(names, range(len(names))))
    idx_e, params_r = get_index_eliminate(W, params_std, TOL_E)
    _check_split(idx_e, ref, "get_index_eliminate")
    assert params_r == [names[i] for i in kept_ref]
    We, params_r2 = eliminate_non_dynaffect(W, params_std, TOL_E)
    assert params_r2 == params_r and We.shape[1] == len(params_r)
    d_sel = lib.DeviceArray((2 + 2 * ncols,), np.int32)
    lib.tsqr_selected(d_W, rows, ldw, lib.DeviceArray.from_host(cs), ncols, TOL_E, 14, 0, -1, None, -1.0, d_sel, None)
    sel = d_sel.to_host()
    assert sel[2:2 + sel[0]].tolist() == kept_ref
    for kw in ({}, dict(fuse=False), dict(chunk_samples=700)):
        _, _, pipe = _pipeline("cfg2_ur10", q, v, a, param=param, **kw)
        for p in range(2):
            _check_split(pipe.run()["idx_e"], ref, "pipeline %s pass %d" % (kw, p))
        if not kw:
            assert pipe.prefix_passes == 1 and pipe.fused_passes == 2


def test_prefix_crossing_refused(lib):
    """UR10 with actuator inertia: joint 2's Ia column below tol_e over the first PREFIX_SAMPLES samples, just above over
    all N.  The first pass refuses the prefix set (prefix_passes 1, fused_passes 0) and returns the exact split; the
    next pass is fused."""
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    P = IdentificationPipeline.PREFIX_SAMPLES
    N = P + 1003
    q, v, a, _ = _straddle_ur10(N, 32, prefix=P)
    param = _param(3)
    robot, coupling, _ = _robot("cfg2_ur10")
    d_W, ldw, ncols, rows, _ = _k1(lib, robot, param, coupling, q, v, a)
    ref = _ld_colsq_device(d_W, rows, ldw, ncols)
    assert ref[14 * 2 + 10] > TOL_E and not rc.undecided(ref, TOL_E, 1e-10)
    # (without the null-pivot rule: a pass the rule cannot certify is repeated, and that repeat runs fused over the set the
    # refused pass learnt -- the counts below are those of the prefix logic alone)
    for null_pivots in (False, True):
        _, _, pipe = _pipeline("cfg2_ur10", q, v, a, param=param, null_pivots=null_pivots)
        _check_split(pipe.run()["idx_e"], ref, "first pass")
        assert pipe.prefix_passes == 1
        if not null_pivots:
            assert pipe.fused_passes == 0
        _check_split(pipe.run()["idx_e"], ref, "second pass")
        assert pipe.fused_passes == (1 if not null_pivots else 1 + pipe.null_rule_fallbacks)


# (cfg, w_layout, chunk_samples): with actuator inertia and friction on, "dense" is the link-compact layout of a wrench
# regressor without the force-compact region (that region takes no friction / inertia columns)
TREE_STRADDLE = [("cfg3_tiago", "block-compact", None), ("cfg3_tiago", "dense", None), ("cfg3_tiago", "dense", 700),
                 ("cfg4_talos", "link-padded", None), ("cfg4_talos", "link-compact", None), ("cfg4_talos", "dense", 700),
                 ("cfg5_human", "dense", None), ("cfg5_human", "link-compact", None), ("cfg5_human", "link-padded", None),
                 ("cfg5_human", "dense", 700)]


@pytest.mark.parametrize("cfg,layout,chunk", TREE_STRADDLE)
def test_copied_columns_at_tol_e_trees(lib, cfg, layout, chunk):
    """Copied columns a hair off tol_e in TIAGo (Ia / fv of joint j in row block j only) and in the external-wrench
    regressors of TALOS and the human model (Ia / fv of LINK k on all six component rows, k the link index into a / v):
    the exact split in both passes of every resident layout and of a chunked pass.  Reference: the long-double norms of
    figh_regressor_build's W (reference layout) and, for a resident pass, of the pass's own W."""
    from conftest import Golden
    g = Golden(cfg)
    robot = g.robot()
    N = 3001
    q, v, a = _inputs(robot, N, [N, 4], "uniform")
    param = dict(g.param, has_friction=True, has_actuator_inertia=True)
    factor = 6 if param["is_external_wrench"] else 1
    picks = np.random.default_rng(3).choice(robot.model.njoints - 1, 6, replace=False)
    cols = {}
    for i, k in enumerate(picks):
        x = a if i % 2 == 0 else v
        side = 1 if i % 3 else -1
        x[:, k], _ = rc.straddle(x[:, k], TOL_E, side, factor=factor)
        cols[14 * int(k) + (10 if i % 2 == 0 else 11)] = side
    d_W, ldw, ncols, rows, _ = _k1(lib, robot, param, False, q, v, a)
    refs = [_ld_colsq_device(d_W, rows, ldw, ncols)]
    d_W.free()
    kw = dict(chunk_samples=chunk) if chunk else dict(w_layout=layout)
    _, _, pipe = _pipeline(cfg, q, v, a, param=param, **kw)
    for p in range(2):
        out = pipe.run()
        if not chunk:
            refs.append(rc.colsq_ld(_pipe_W(pipe, N)))
        for ref in refs:
            for c, side in cols.items():
                assert (ref[c] > TOL_E) == (side > 0), "column %d not where the inputs put it" % c
            assert not rc.undecided(ref, TOL_E, 1e-10)
            _check_split(out["idx_e"], ref, "%s %s chunk %s pass %d" % (cfg, layout, chunk, p))


def test_tx40_coupling_columns_at_tol_e(lib):
    """TX40: the coupling columns carry a5 / a4 (Iam6) and v5 / v4 (fvm6) on row blocks 4 and 5 (oracle_np.add_coupling_TX40),
    joints 4 and 5's Ia / fv columns one of them each.  a4, a5 at 0.5 tol_e (1 + 1e-9) each -- Iam6 just above tol_e, Ia4 and
    Ia5 at half of it -- and v4, v5 at 0.5 tol_e (1 - 1e-9): fvm6 just below.  The exact split in get_index_eliminate on the
    kernel's W and in both passes of the pipeline, fuse=False and chunk_samples."""
    from conftest import Golden
    from figaroh_plus_amd.tools.regressor import get_index_eliminate
    g = Golden("cfg1_tx40")
    robot = g.robot()
    N = 3001
    q, v, a = _inputs(robot, N, [N, 40], "uniform")
    for x, side in ((a, 1), (v, -1)):
        for j in (4, 5):
            x[:, j], _ = rc.scale_to_norm(x[:, j], 0.5 * TOL_E * (1 + side * 1e-9))
    d_W, ldw, ncols, rows, _ = _k1(lib, robot, g.param, True, q, v, a)
    assert ncols == 87
    W = d_W.to_host().reshape(rows, ldw)
    ref = rc.colsq_ld(W)
    for c, side in ((84, 1), (85, -1)):
        rel = float((ref[c] - np.longdouble(TOL_E)) / np.longdouble(TOL_E))
        assert side * rel >= 0.99e-9, "coupling column %d: %.3e" % (c, rel)
    assert all(ref[14 * j + s] < 0.6 * TOL_E for j in (4, 5) for s in (10, 11))
    assert not rc.undecided(ref, TOL_E, 1e-10)
    params_std = dict(zip(g.params_std().keys(), range(ncols)))
    _check_split(get_index_eliminate(W, params_std, TOL_E)[0], ref, "get_index_eliminate")
    for kw in ({}, dict(fuse=False), dict(chunk_samples=700)):
        _, _, pipe = _pipeline("cfg1_tx40", q, v, a, **kw)
        for p in range(2):
            _check_split(pipe.run()["idx_e"], ref, "pipeline %s pass %d" % (kw, p))


def _inertia_column(ref, nl):
    """The inertia-tensor column (slots 0 .. 5) of the last link with one, largest norm first."""
    for link in range(nl - 1, -1, -1):
        c = 14 * link + np.arange(6)
        if (ref[c] > 0).any():
            return int(c[np.argmax(np.asarray(ref[c], dtype=np.float64))])
    raise AssertionError("no inertia column")


@pytest.mark.parametrize("side", [-1, 1])
@pytest.mark.parametrize("cfg", ["cfg2_ur10", "cfg4_talos"])
def test_computed_columns_at_tol_e(lib, cfg, side, record_property):
    """A computed column at tol_e (1 +- 1e-6): a near-static motion (v = 0, so the inertia-tensor columns are linear in a),
    a scaled so that the long-double norm of an inertia-tensor column of the last link lands there -- measured on the
    kernel's own W, the margin absorbing the differences in W between paths.  The exact split in the drop-in
    get_index_eliminate and in both passes of the pipeline: UR10 (prefix + fused, fuse=False, chunk_samples), TALOS
    force-compact and link-padded (the golden param: no friction / inertia columns, so the force-compact region is used)."""
    from conftest import Golden
    from figaroh_plus_amd.tools.regressor import get_index_eliminate
    g = Golden(cfg)
    robot = g.robot()
    N = 5003 if cfg == "cfg2_ur10" else 3001
    q, v, a = _inputs(robot, N, [N, 41], "uniform")
    v[:] = 0.0
    d_W, ldw, ncols, rows, _ = _k1(lib, robot, g.param, g.coupling, q, v, a)
    ref0 = _ld_colsq_device(d_W, rows, ldw, ncols)
    c = _inertia_column(ref0, robot.model.njoints - 1)
    a *= np.sqrt(float(TOL_E * (1 + side * 1e-6) / ref0[c]))
    d_W, ldw, ncols, rows, _ = _k1(lib, robot, g.param, g.coupling, q, v, a)
    W = d_W.to_host().reshape(rows, ldw)
    refs = [rc.colsq_ld(W)]
    rel = float((refs[0][c] - np.longdouble(TOL_E)) / np.longdouble(TOL_E))
    record_property("computed_%s_%+d:rel_to_tol_e" % (cfg, side), "%.3e" % rel)
    params_std = dict(zip(g.params_std().keys(), range(ncols)))
    _check_split(get_index_eliminate(W, params_std, TOL_E)[0], refs[0], "get_index_eliminate")
    del W
    cases = ({}, dict(fuse=False), dict(chunk_samples=700)) if cfg == "cfg2_ur10" else (
        dict(w_layout="dense"), dict(w_layout="link-padded"))
    for kw in cases:
        _, _, pipe = _pipeline(cfg, q, v, a, **kw)
        for p in range(2):
            out = pipe.run()
            own = [] if "chunk_samples" in kw else [rc.colsq_ld(_pipe_W(pipe, N))]
            if p == 0 and kw.get("w_layout") == "dense":
                assert getattr(pipe.W, "force_ld", 0) > 0  # (the force-compact layout)
            for ref in refs + own:
                r = float((ref[c] - np.longdouble(TOL_E)) / np.longdouble(TOL_E))
                assert side * r >= 0.5e-6, "column %d at %.3e of tol_e in %s" % (c, r, kw)
                assert [k for k in rc.undecided(ref, TOL_E, 1e-9) if k != c] == []
                _check_split(out["idx_e"], ref, "%s %s pass %d" % (cfg, kw, p))


def _sharded_outs(robot, param, q, v, a, tau, world, layout="dense", coupling=False):
    """One IdentificationPipeline per shard (``world`` equal shards) under tools/fuzz_sharded.ReplayExchange: rounds of the
    same pass until every rank has seen every other rank's contribution.  Returns the last round's outputs."""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from fuzz_sharded import ReplayExchange
    N = len(q)
    rps = tau.shape[0] // N
    bounds = np.linspace(0, N, world + 1).astype(int)
    board, pipes = {}, []
    for r in range(world):
        lo, hi = bounds[r], bounds[r + 1]
        ex = ReplayExchange(board, r, world)
        tau_r = np.concatenate([tau[j * N + lo:j * N + hi] for j in range(rps)])
        pipes.append((_pipeline_of(robot, param, q[lo:hi], v[lo:hi], a[lo:hi], tau_r, w_layout=layout, exchange=ex,
                                   coupling=coupling), ex))
    outs = None
    for _ in range(5):
        outs = []
        for p, ex in pipes:
            ex.new_round()
            try:
                outs.append(p.run())
            except ValueError:  # (a rank that has only seen zeros of the others in round 0)
                outs.append(None)
    assert all(o is not None for o in outs), "a rank did not settle"
    return outs, bounds


@pytest.mark.parametrize("cfg,layout,world", [("cfg2_ur10", "dense", 3), ("cfg3_tiago", "block-compact", 2)])
def test_shards_sum_crosses_tol_e(lib, cfg, layout, world):
    """Samples split into shards (tools/fuzz_sharded.ReplayExchange): a copied column below tol_e on every shard but just
    above it in total is kept, one just below in total is eliminated -- the decision is taken on the all-reduced norms
    (sum_columns_device, then select_columns; for the chain also in the prefix pass of _learn_kept_set), not on a rank's
    own.  Every rank returns the exact split of all samples."""
    from conftest import Golden
    g = Golden(cfg)
    robot = g.robot()
    N = 3 * 4500 if cfg == "cfg2_ur10" else 2 * 1601
    q, v, a = _inputs(robot, N, [N, world], "uniform")
    param = dict(g.param, has_friction=True, has_actuator_inertia=True)
    bounds = np.linspace(0, N, world + 1).astype(int)
    for x, j, side in ((a, 2, 1), (v, 3, -1)):
        for r in range(world):  # every shard at tol_e / world: below tol_e on its own
            sl = slice(bounds[r], bounds[r + 1])
            x[sl, j], _ = rc.scale_to_norm(x[sl, j], TOL_E * (1 + side * 1e-9) / world)
    d_W, ldw, ncols, rows, _ = _k1(lib, robot, param, False, q, v, a)
    W = d_W.to_host().reshape(rows, ldw)
    ref = rc.colsq_ld(W)
    kept_c, gone_c = 14 * 2 + 10, 14 * 3 + 11
    assert ref[kept_c] > TOL_E * (1 + 0.99e-9) and ref[gone_c] < TOL_E * (1 - 0.99e-9)
    assert not rc.undecided(ref, TOL_E, 1e-10)
    for r in range(world):
        rows_r = np.concatenate([np.arange(j * N + bounds[r], j * N + bounds[r + 1]) for j in range(rows // N)])
        assert rc.colsq_ld(W[rows_r][:, [kept_c]])[0] < TOL_E
    tau = W @ np.ones(ncols) + 0.01 * np.random.default_rng(5).standard_normal(rows)
    del W
    outs, _ = _sharded_outs(robot, param, q, v, a, tau, world, layout)
    for r, o in enumerate(outs):
        _check_split(o["idx_e"], ref, "%s rank %d of %d" % (cfg, r, world))
        assert kept_c not in o["idx_e"] and gone_c in o["idx_e"]


@pytest.mark.parametrize("cfg", ["cfg2_ur10", "cfg3_tiago"])
def test_tol_e_sweep(lib, cfg):
    """tol_e = cs*_j (1 +- delta) for the smallest non-zero, a middle and the largest column of the golden inputs: the split
    flips at exactly that column.  delta = 2 gamma_m for get_index_eliminate on the W the reference was summed from; plus
    the sibling slack for the pipeline's pass (its own K1)."""
    from conftest import Golden
    from figaroh_plus_amd.tools.regressor import get_index_eliminate
    g = Golden(cfg)
    robot = g.robot()
    q, v, a = g["q_big"], g["v_big"], g["a_big"]
    d_W, ldw, ncols, rows, _ = _k1(lib, robot, g.param, g.coupling, q, v, a)
    W = d_W.to_host().reshape(rows, ldw)
    ref = rc.colsq_ld(W)
    nz = np.flatnonzero(ref > 0)
    order = nz[np.argsort(np.asarray(ref[nz], dtype=np.float64))]
    params_std = dict(zip(g.params_std().keys(), range(ncols)))
    checked = 0
    for j in [order[0], order[len(order) // 2], order[-1]]:
        for slack, path in ((0.0, "dropin"), (SIBLING_SLACK, "pipeline")):
            delta = 2 * rc.gamma(rows) + slack
            for side in (-1, 1):
                tol = float(ref[j]) * (1 + side * delta)
                if [c for c in rc.undecided(ref, tol, 2 * delta) if c != j]:
                    continue  # another column this close to the threshold: no exact split to compare with
                expect = rc.exact_split(ref, tol)[0]
                assert (j in expect) == (side > 0)
                if path == "dropin":
                    assert get_index_eliminate(W, params_std, tol)[0] == expect
                elif len(expect) == ncols:  # (the largest column just below tol_e: the pipeline refuses to go on)
                    _, _, pipe = _pipeline(cfg, q, v, a, tol_e=tol)
                    with pytest.raises(ValueError, match="every column"):
                        pipe.run()
                else:
                    _, _, pipe = _pipeline(cfg, q, v, a, tol_e=tol)
                    assert pipe.run()["idx_e"] == expect
                checked += 1
    assert checked >= 8


# ---------------------------------------------------------------------------------------------------- 4. gram and sigma2
@pytest.mark.parametrize("cfg,N", [("cfg2_ur10", 1501), ("cfg3_tiago", 301)])
def test_regressor_gram_entrywise(lib, cfg, N, record_property):
    """figh_regressor_gram (G, W^T tau, tau^T tau from the streamed triangle) entry by entry against the long-double Gram of
    the same samples' W: |G_ij - G*_ij| <= TOL_BACKWARD |w_i| |w_j|, |g_i - g*_i| <= TOL_BACKWARD |w_i| |tau|, tau^T tau
    relative; chunk_samples 0, 64, 150."""
    from conftest import Golden
    from figaroh_plus_amd.tools.regressor import _samples_to_device, regressor_flags
    g = Golden(cfg)
    robot = g.robot()
    q, v, a = _inputs(robot, N, 12, "distal")
    d_W, ldw, ncols, rows, _ = _k1(lib, robot, g.param, g.coupling, q, v, a)
    W = d_W.to_host().reshape(rows, ldw)[:, :ncols]
    kept = np.flatnonzero(np.asarray(rc.colsq_ld(W), dtype=np.float64) >= TOL_E).astype(np.int32)
    rng = np.random.default_rng(2)
    tau = W[:, kept] @ rng.standard_normal(len(kept)) + 1e-3 * rng.standard_normal(rows)
    A = np.asarray(np.c_[W[:, kept], tau], dtype=np.longdouble)
    Gl = A.T @ A
    nrm = np.sqrt(np.asarray(np.diag(Gl), dtype=np.float64))
    n = len(kept)
    mode, flags, ft = regressor_flags(g.param, g.coupling)
    _, d_q, d_v, d_a = _samples_to_device(robot.model, q, v, a)
    worst = 0.0
    for chunk in [0, 64, 150]:
        G, gv, tt = lib.regressor_gram(robot.device_model(), mode, flags, ft, N, d_q, d_v, d_a,
                                       lib.DeviceArray.from_host(kept), n, lib.DeviceArray.from_host(tau), chunk)
        EG = np.abs(np.asarray(G, dtype=np.longdouble) - Gl[:n, :n]) / np.outer(nrm[:n], nrm[:n])
        Eg = np.abs(np.asarray(gv, dtype=np.longdouble) - Gl[:n, n]) / (nrm[:n] * nrm[n])
        Et = abs(np.longdouble(tt) - Gl[n, n]) / Gl[n, n]
        w = float(max(EG.max(), Eg.max(), Et)) / TOL_BACKWARD
        worst = max(worst, w)
        assert w <= 1.0, "%s chunk %d: %.3g TOL_BACKWARD" % (cfg, chunk, w)
    record_property("gram_%s:over_bound" % cfg, "%.3e" % worst)


def _noisy_tau(W, phi, nblk, N, rng):
    """tau = W phi + per-joint noise from 1e-6 to 1e-1 of that joint's torque scale (rms)."""
    tau = W @ phi
    lev = np.logspace(-6, -1, nblk)
    rng.shuffle(lev)
    for j in range(nblk):
        sl = slice(j * N, (j + 1) * N)
        scale = float(np.sqrt(np.mean(tau[sl] ** 2))) or 1.0
        tau[sl] += lev[j] * scale * rng.standard_normal(N)
    return tau, lev


@pytest.mark.parametrize("cfg,layout", [("cfg2_ur10", "dense"), ("cfg4_talos", "dense"), ("cfg3_tiago", "block-compact"),
                                        ("cfg3_tiago", "dense")])
def test_sigma2_joint_by_joint(lib, cfg, layout, record_property):
    """sigma2_joint of run(wls=True) joint by joint against the long-double ||tau_j - W_b,j phi_b||^2 / n_j of the pass's own
    W.  "second pass over W" (figh_matvec + figh_block_sqnorm): the a-priori direct bound.  "per-row-block triangles"
    (TIAGo): the same bound with the triangle's column-wise backward error (TOL_BACKWARD sum_c |a_j,c| |v_c|) in place of
    e_j; the looser bound of the Gram metric alone is recorded beside it."""
    from conftest import Golden
    g = Golden(cfg)
    robot = g.robot()
    N = 4001
    q, v, a = _inputs(robot, N, [N, 6], "uniform")
    d_W, ldw, ncols, rows, _ = _k1(lib, robot, g.param, g.coupling, q, v, a)
    W0 = d_W.to_host().reshape(rows, ldw)[:, :ncols]
    d_W.free()
    nblk = rows // N
    tau, lev = _noisy_tau(W0, g.phi_ref(), nblk, N, np.random.default_rng(17))
    del W0
    _, _, pipe = _pipeline(cfg, q, v, a, tau=tau, w_layout=layout)
    pipe.run(wls=True)
    out = pipe.run(wls=True)
    W = _pipe_W(pipe, N)
    kept = [i for i in range(ncols) if i not in set(out["idx_e"])]
    Wb = W[:, kept][:, np.asarray(out["idx_base"])]
    phi = np.asarray(out["phi_b"], dtype=np.float64)
    y = np.asarray(Wb, dtype=np.longdouble) @ np.asarray(phi, dtype=np.longdouble)
    n_j = [N] * nblk
    ref = rc.sigma2_ld(tau, y, n_j)
    r_norm = np.sqrt(ref * N)
    err = np.abs(np.asarray(out["sigma2_joint"], dtype=np.longdouble) - ref)
    tag = "sigma2_%s_%s" % (cfg, layout)
    if out["wls_source"] == "second pass over W":
        ratio = np.asarray(err / rc.sigma2_direct_bound(tau, Wb, phi, n_j, r_norm), dtype=np.float64)
        record_property(tag + ":direct_over_bound", "%.3e" % ratio.max())
        assert (ratio <= 1.0).all(), "%s: joints %s above the bound (%s)" % (tag, np.flatnonzero(ratio > 1).tolist(), ratio)
    else:
        assert out["wls_source"] == "per-row-block triangles"
        A_norms = [np.r_[np.sqrt(np.asarray(rc.colsq_ld(Wb[j * N:(j + 1) * N]), dtype=np.float64)),
                         float(np.linalg.norm(tau[j * N:(j + 1) * N]))] for j in range(nblk)]
        tight, loose = rc.sigma2_triangle_bounds(A_norms, np.r_[phi, -1.0], r_norm, len(kept) + 1, n_j, TOL_BACKWARD)
        e = np.asarray(err, dtype=np.float64)
        record_property(tag + ":triangle_over_tight", "%.3e" % (e / tight).max())
        record_property(tag + ":triangle_over_loose", "%.3e" % (e / loose).max())
        assert (e <= tight).all(), "%s: joints %s above the tight bound (%s)" % (
            tag, np.flatnonzero(e > tight).tolist(), (e / tight)[e > tight])
    # (the precise joint, noise 1e-6 of its torque scale, is read at its own scale -- not at 1e-9 of the largest variance)
    jp = int(np.argmin(lev))
    record_property(tag + ":precise_joint_rel", "%.3e" % float(err[jp] / ref[jp]))
