"""GPU suite: the HIP path (through the C-ABI) against the oracle and the golden vectors.

Tolerances: integer / index / string results are compared exactly; regressor entries to 1e-12 of the
matrix scale (the reference's own inner kernel, Pinocchio, is unpinned: oracle header); parameter
estimates to 1e-6 relative (BASELINE.json north_star) or to the reference's own 6-decimal rounding.
"""
import contextlib
import io
import json
import os

import numpy as np
import pytest

import oracle_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    return _lib


def _free_port_pair():
    """A port p with p + 101 free as well (the socket control plane of dist.SocketGroup listens on MASTER_PORT + 101)."""
    import socket
    for _ in range(50):
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        try:
            with socket.socket() as s2:
                s2.bind(("127.0.0.1", port + 101))
            return port
        except (OSError, OverflowError):
            continue
    raise RuntimeError("no free port pair")


def _oracle_W(g, oracle_lib, q, v, a, param=None, coupling=None):
    om = oracle_lib.OracleModel(g.flat())
    mode, flags, ft = oracle_lib.param_flags(param or g.param, g.coupling if coupling is None else coupling)
    return om.build_regressor_basic(q, v, a, mode, flags, ft)


def _gpu_W(g, q, v, a, param=None, coupling=None, generic=False):
    from figaroh_plus_amd.tools.regressor import add_coupling_TX40, build_regressor_basic
    robot = g.robot()
    p = dict(param or g.param)
    if generic:
        p["force_generic_kernel"] = True
    W = build_regressor_basic(robot, q, v, a, p)
    if g.coupling if coupling is None else coupling:
        m = robot.model
        W = add_coupling_TX40(W, m, robot.data, len(q), m.nq, m.nv, m.njoints, q, v, a)
    return W


# ------------------------------------------------------------------------------------------------ K1
def test_regressor_matches_golden(lib, golden):
    g = golden
    W = _gpu_W(g, g["q_small"], g["v_small"], g["a_small"])
    ref = g["W_small"]
    assert W.shape == ref.shape and W.dtype == np.float64
    assert np.abs(W - ref).max() <= 1e-12 * np.abs(ref).max()
    # structural zeros (and sign(0) = 0) are exact: wherever the reference is exactly zero, so is the kernel.  The other
    # direction holds up to rounding residues of the REFERENCE's own arithmetic: Pinocchio's literal propagation of the
    # 6 x 10 body regressor leaves entries of 1e-17 relative size (TIAGo: mz of two links on the prismatic torso row)
    # where the closed-form row evaluation of the tree kernel gives an exact zero.
    assert not W[ref == 0].any()
    extra_zero = (W == 0) & (ref != 0)
    assert np.abs(ref[extra_zero]).max(initial=0.0) <= 1e-15 * np.abs(ref).max()


def test_generic_tree_kernel_on_chains(lib, golden):
    if golden.name not in ("cfg1_tx40", "cfg2_ur10"):
        pytest.skip("chain robots only")
    g = golden
    W = _gpu_W(g, g["q_small"], g["v_small"], g["a_small"], generic=True)
    assert np.abs(W - g["W_small"]).max() <= 1e-12 * np.abs(g["W_small"]).max()


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_regressor_ragged_sizes(lib, golden, oracle_lib, N):
    g = golden
    if N == 1000 and golden.name in ("cfg3_tiago",):
        N = 200
    rng = np.random.default_rng(N)
    reps = -(-N // len(g["q_big"]))
    q = np.tile(g["q_big"], (reps, 1))[:N]
    v = rng.uniform(-2, 2, (N, g.meta["dims"]["nv"]))
    a = rng.uniform(-5, 5, (N, g.meta["dims"]["nv"]))
    W = _gpu_W(g, q, v, a)
    ref = _oracle_W(g, oracle_lib, q, v, a)
    if g.coupling:
        pass  # oracle flag 8 already appended the coupling columns
    assert W.shape == ref.shape
    assert np.abs(W - ref).max() <= 1e-12 * np.abs(ref).max()


def test_tx40_fused_coupling_equals_appended(lib, golden_tx40):
    from figaroh_plus_amd.tools.regressor import build_regressor_device
    from figaroh_plus_amd import _lib
    g = golden_tx40
    robot = g.robot()
    q, v, a = g["q_small"], g["v_small"], g["a_small"]
    dq, dv, da = (_lib.DeviceArray.from_host(np.ascontiguousarray(x).reshape(-1)) for x in (q, v, a))
    W, colsq = build_regressor_device(robot, dq, dv, da, len(q), g.param, coupling=True, colsq=True)
    Wh = W.numpy()
    assert Wh.shape == (6 * len(q), 87)
    assert np.abs(Wh - g["W_small"]).max() <= 1e-12 * np.abs(g["W_small"]).max()
    cs = colsq.to_host()
    ref = np.einsum("ij,ij->j", g["W_small"], g["W_small"])
    assert np.abs(cs - ref).max() <= 1e-12 * ref.max()


def test_external_wrench_component_selection(lib, oracle_lib):
    from conftest import Golden
    g = Golden("cfg5_human")
    param = dict(g.param, force_torque=["Fx", "Mz"], has_friction=True, has_actuator_inertia=True, has_joint_offset=True)
    q, v, a = g["q_small"], g["v_small"], g["a_small"]
    W = _gpu_W(g, q, v, a, param=param)
    ref = _oracle_W(g, oracle_lib, q, v, a, param=param)
    assert np.abs(W - ref).max() <= 1e-12 * np.abs(ref).max()
    N = len(q)
    assert not W[N:3 * N, :10].any() and W[:N, :10].any()
    bad = dict(param, force_torque=["Fq"])
    with pytest.raises(ValueError, match="Please enter valid parameters"):
        _gpu_W(g, q, v, a, param=bad)


def test_shape_errors(lib, golden_ur10):
    from figaroh_plus_amd.tools.regressor import build_regressor_basic
    g = golden_ur10
    with pytest.raises(ValueError):
        build_regressor_basic(g.robot(), g["q_small"], g["v_small"][:, :5], g["a_small"], g.param)
    W = build_regressor_basic(g.robot(), np.zeros((0, 6)), np.zeros((0, 6)), np.zeros((0, 6)), g.param)
    assert W.shape == (0, 84)


# ------------------------------------------------------------------------------------------------ K2 + drop-in API
def test_elimination_functions(lib, golden, oracle_lib):
    from figaroh_plus_amd.tools.regressor import build_regressor_reduced, eliminate_non_dynaffect, get_index_eliminate
    g = golden
    W = _gpu_W(g, g["q_big"], g["v_big"], g["a_big"])
    idx_e, params_r = get_index_eliminate(W, g.params_std(), 1e-6)
    assert idx_e == list(g["idx_e"]) and params_r == g.meta["params_r"]
    W_e = build_regressor_reduced(W, idx_e)
    assert np.array_equal(W_e, np.delete(W, idx_e, 1))
    W_e2, params_r2 = eliminate_non_dynaffect(W, g.params_std(), 1e-6)
    assert params_r2 == params_r and np.array_equal(W_e2, W_e)
    # every column eliminated / none eliminated
    assert get_index_eliminate(W, g.params_std(), 1e300)[0] == list(range(W.shape[1]))
    assert build_regressor_reduced(W, []).shape == W.shape


def test_base_parameters_identical(lib, golden):
    from figaroh_plus_amd.tools.qrdecomposition import build_baseRegressor, get_baseIndex, get_baseParams
    g = golden
    W = _gpu_W(g, g["q_big"], g["v_big"], g["a_big"])
    W_e = np.delete(W, g["idx_e"], 1)
    W_b, params_base, idx_base = get_baseParams(W_e, g.meta["params_r"], g.params_std())
    assert idx_base == list(g["idx_base"])
    assert params_base == g.meta["params_base"]
    assert np.array_equal(W_b, W_e[:, idx_base])
    assert get_baseIndex(W_e, g.meta["params_r"]) == tuple(idx_base)
    assert np.array_equal(build_baseRegressor(W_e, tuple(idx_base)), W_b)
    with pytest.raises(AssertionError):
        get_baseIndex(W_e, g.meta["params_r"][:-1])


def test_double_qr_and_sigma(lib, golden):
    from figaroh_plus_amd.identification.identification_tools import least_squares, relative_stdev
    from figaroh_plus_amd.tools.qrdecomposition import cond_num, double_QR
    g = golden
    W = _gpu_W(g, g["q_big"], g["v_big"], g["a_big"])
    W_e = np.delete(W, g["idx_e"], 1)
    std = {k: float(x) for k, x in g.params_std().items()}
    W_b, base_parameters, params_base, phi_b, phi_std = double_QR(g["tau"], W_e, g.meta["params_r"], std)
    assert params_base == g.meta["params_base"]
    assert list(base_parameters.keys()) == params_base
    scale = max(1.0, np.abs(g["phi_b"]).max())
    assert np.abs(phi_b - g["phi_b"]).max() <= 1.5e-6 * scale      # both rounded to 6 decimals
    assert np.abs(phi_std - g["phi_std"]).max() <= 2e-5 * max(1.0, np.abs(g["phi_std"]).max())
    assert len(double_QR(g["tau"], W_e, g.meta["params_r"])) == 4
    phi = least_squares(W_b, g["tau"])
    assert np.abs(phi - g["phi_pinv"]).max() <= 1e-6 * np.abs(g["phi_pinv"]).max()   # north-star tolerance
    s = relative_stdev(W_b, g["phi_b"], g["tau"])
    assert np.abs(s - g["std_ols"]).max() <= 0.011 + 1e-6 * np.abs(g["std_ols"]).max()
    c = cond_num(W_b)
    assert abs(c - g["cond_Wb"][0]) <= 1e-7 * g["cond_Wb"][0]
    assert abs(cond_num(W_b, "max_over_min_sigma") - g["cond_Wb"][1]) <= 1e-6 * g["cond_Wb"][1]
    with pytest.raises(np.linalg.LinAlgError):
        cond_num(W_b, "fro")


def test_weighted_least_squares(lib, golden):
    from figaroh_plus_amd.identification.identification_tools import weighted_least_squares_blocks, weigthed_least_squares
    g = golden
    if "phi_wls_script" not in g.z.files:
        pytest.skip("no WLS golden")
    W = _gpu_W(g, g["q_big"], g["v_big"], g["a_big"])
    W_b = np.delete(W, g["idx_e"], 1)[:, g["idx_base"]]
    nblk = g.meta["dims"]["nv"] if g.param["is_joint_torques"] else 6
    phi, std = weighted_least_squares_blocks(W_b, g["tau"], g["phi_b"], nblk)
    assert np.abs(phi - g["phi_wls_script"]).max() <= 1.5e-6 * max(1.0, np.abs(phi).max())
    big = np.abs(g["std_wls_script"]) < 1e4
    assert np.abs(std - g["std_wls_script"])[big].max() <= 0.011 + 1e-5 * np.abs(g["std_wls_script"][big]).max()
    if "phi_wls_lib" in g.z.files:
        n = len(g["tau"]) // nblk
        param = dict(g.param, idx_tau_stop=[(b + 1) * n for b in range(nblk)])

        class R:  # the reference reads robot.model.nq as the number of joint blocks
            pass
        r = R()
        r.model = R()
        r.model.nq = nblk
        phi2 = weigthed_least_squares(r, g["phi_b"], W_b, g["tau"], W_b @ g["phi_b"], param)
        assert np.abs(phi2 - g["phi_wls_lib"]).max() <= 1.5e-6 * max(1.0, np.abs(phi2).max())


# ------------------------------------------------------------------------------------------------ K3 properties
def test_tsqr_gram_identity_and_permutation(lib, golden):
    from figaroh_plus_amd.tools.qrdecomposition import rfactor
    g = golden
    W = _gpu_W(g, g["q_big"], g["v_big"], g["a_big"])
    keep = [i for i in range(W.shape[1]) if i not in set(g["idx_e"].tolist())]
    R = rfactor(W, col_idx=keep)
    G = W[:, keep].T @ W[:, keep]
    assert np.abs(R.T @ R - G).max() <= 1e-12 * np.abs(G).max()
    assert np.array_equal(R, np.triu(R))
    Wb = W[:, keep][:, g["idx_base"]]
    Rb = rfactor(Wb)
    ref = np.linalg.qr(Wb, mode="r")
    assert np.abs(np.abs(np.diag(Rb)) - np.abs(np.diag(ref))).max() <= 1e-10 * np.abs(np.diag(ref)).max()
    perm = np.random.default_rng(1).permutation(Wb.shape[0])
    Rp = rfactor(np.ascontiguousarray(Wb[perm]))
    assert np.abs(np.abs(Rp) - np.abs(Rb)).max() <= 1e-10 * np.abs(Rb).max()
    # tau column: Q^T tau and the residual norm
    Ra = rfactor(Wb, tau=g["tau"])
    phi = np.linalg.solve(Ra[:-1, :-1], Ra[:-1, -1])
    ref_phi, res, _, _ = np.linalg.lstsq(Wb, g["tau"], rcond=None)
    assert np.abs(phi - ref_phi).max() <= 1e-9 * np.abs(ref_phi).max()
    assert abs(abs(Ra[-1, -1]) - np.sqrt(res[0])) <= 1e-9 * np.sqrt(res[0])


def test_tsqr_merge_equals_one_shot(lib, golden_ur10):
    from figaroh_plus_amd import _lib
    from figaroh_plus_amd.tools.qrdecomposition import rfactor
    g = golden_ur10
    W = _gpu_W(g, g["q_big"], g["v_big"], g["a_big"])
    keep = [i for i in range(84) if i not in set(g["idx_e"].tolist())]
    We = np.ascontiguousarray(W[:, keep])
    N = len(g["q_big"])
    parts = []
    for lo, hi in ((0, 150), (150, 400)):
        rows = np.concatenate([np.arange(j * N + lo, j * N + hi) for j in range(6)])
        parts.append(rfactor(np.ascontiguousarray(We[rows])))
    d_stack = _lib.DeviceArray.from_host(np.stack(parts).reshape(-1))
    d_R = _lib.DeviceArray((49 * 49,))
    _lib.tsqr_merge(d_stack, 2, 49, d_R)
    Rm = np.triu(d_R.to_host().reshape(49, 49))
    G = We.T @ We
    assert np.abs(Rm.T @ Rm - G).max() <= 1e-12 * np.abs(G).max()
    d = np.abs(np.diag(Rm))
    assert [i for i in range(49) if d[i] > 1e-8] == list(g["idx_base"])


# ------------------------------------------------------------------------------------------------ pipeline
def test_pipeline_matches_reference_outputs(lib, golden):
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    g = golden
    pipe = IdentificationPipeline(g.robot(), g.param, params_std=g.params_std(), coupling=g.coupling)
    pipe.set_samples(g["q_big"], g["v_big"], g["a_big"], g["tau"])
    out = pipe.run()
    assert out["idx_e"] == list(g["idx_e"])
    assert out["params_r"] == g.meta["params_r"]
    assert out["idx_base"] == list(g["idx_base"])
    assert out["params_base"] == g.meta["params_base"]
    assert np.abs(out["col_norm"] - g["colsq_big"]).max() <= 1e-12 * g["colsq_big"].max()
    assert np.abs(out["phi_ls"] - g["phi_pinv"]).max() <= 1e-6 * np.abs(g["phi_pinv"]).max()
    assert np.abs(out["phi_b"] - g["phi_b"]).max() <= 1.5e-6 * max(1.0, np.abs(g["phi_b"]).max())
    out2 = pipe.run()  # second pass reuses the HBM buffers: idempotent
    assert out2["idx_base"] == out["idx_base"] and np.array_equal(out2["phi_b"], out["phi_b"])


@pytest.mark.parametrize("cfg,N", [("cfg2_ur10", 10 ** 6), ("cfg1_tx40", 50000)])
def test_full_size_structural_invariants(lib, cfg, N, oracle_lib):
    """BASELINE.json sizes: the base-parameter expressions are structural, so at 1e6 samples they must
    be the committed strings; W . phi_urdf must equal the torque model; spot rows equal the oracle."""
    from conftest import Golden
    from figaroh_plus_amd import _lib
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    g = Golden(cfg)
    rng = np.random.default_rng(20250410 + (2 if cfg == "cfg2_ur10" else 1))
    qr, vr, ar = (6, 6, 6) if cfg == "cfg2_ur10" else (6, 10, 30)
    q, v, a = rng.uniform(-qr, qr, (N, 6)), rng.uniform(-vr, vr, (N, 6)), rng.uniform(-ar, ar, (N, 6))
    pipe = IdentificationPipeline(g.robot(), g.param, params_std=g.params_std(), coupling=g.coupling)
    pipe.set_samples(q, v, a)
    phi = g.phi_ref()
    pipe.set_tau_from_parameters(phi)
    out = pipe.run()
    assert out["idx_e"] == list(g["idx_e"])
    if cfg == "cfg2_ur10":
        assert out["idx_base"] == list(g["idx_base"])
        assert out["params_base"] == g.meta["params_base"]
        # noise-free tau = W phi_ref: the identified base parameters are the regrouped standard ones
        assert np.abs(out["phi_ls"] - g["phi_from_std"]).max() <= 1e-6 * np.abs(g["phi_from_std"]).max()
        # the null-pivot rule stays certified at the BASELINE size (sqrt(T) margin of _host.null_rule_certified)
        assert out["null_rule_certified"] and pipe.null_rule_fallbacks == 0
    else:
        # TX40 at the script's 50 000 samples: one structurally dependent pivot is a genuine tiny number that
        # grows like sqrt(N) (2.5e-9 at N=400, 2.7e-8 here) and crosses TOL_QR=1e-8, so the REFERENCE's own
        # np.linalg.qr keeps 62 columns at this size.  Parity = the same decision as LAPACK on the same rows.
        W_ref = _oracle_W(g, oracle_lib, q, v, a)
        keep = [i for i in range(W_ref.shape[1]) if i not in set(out["idx_e"])]
        d = np.abs(np.diag(np.linalg.qr(W_ref[:, keep], mode="r")))
        ref_base = [i for i in range(len(keep)) if d[i] > 1e-8]
        assert len(ref_base) == 62
        assert out["idx_base"] == ref_base
        dep = [i for i in range(len(keep)) if i not in set(ref_base)]
        assert out["absdiagR"][dep].max() < 1e-9 and out["absdiagR"][ref_base].min() > 1e-8
    assert out["residual_norm"] <= 1e-9 * np.sqrt(out["rows"]) * max(1.0, np.abs(phi).max()) * 1e3
    # spot-check 257 scattered samples of the HBM-resident W against the oracle
    sel = rng.choice(N, 257, replace=False)
    Wsel = _oracle_W(g, oracle_lib, q[sel], v[sel], a[sel])
    rows = np.concatenate([j * N + sel for j in range(6)])
    W = pipe.W
    d_idx = _lib.DeviceArray.from_host(np.arange(W.cols, dtype=np.int32))
    host_rows = np.empty((len(rows), W.cols))
    for k, r in enumerate(rows):  # row gather through the ABI: d2h of one row each
        _lib.check(_lib.load().figh_memcpy_d2h(host_rows[k].ctypes.data, W.buf.ptr + int(r) * W.ld * 8, W.cols * 8))
    assert np.abs(host_rows - Wsel).max() <= 1e-12 * np.abs(Wsel).max()


def _tree_pipeline(cfg, N, seed, chunk=None, tau=True):
    from conftest import Golden
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    g = Golden(cfg)
    robot = g.robot()
    q, v, a = sample_inputs(robot.model, N, np.random.default_rng(seed), 1.5, 2, 5)
    pipe = IdentificationPipeline(robot, g.param, params_std=g.params_std(), coupling=g.coupling, chunk_samples=chunk)
    pipe.set_samples(q, v, a)
    if tau:
        pipe.set_tau_from_parameters(g.phi_ref())
    return g, pipe, (q, v, a)


def _spot_rows_padded(pipe, g, oracle_lib, qva, rps, rng):
    """Scattered samples of the HBM-resident, LINK-PADDED W (16 columns per link) against the oracle: the 14 reference
    columns of every link agree, the two padding columns are exactly zero."""
    from figaroh_plus_amd import _lib
    q, v, a = qva
    N = len(q)
    sel = np.unique(np.concatenate([rng.choice(N, 61, replace=False), [0, 63, 64, N - 65, N - 64, N - 1]]))
    Wsel = _oracle_W(g, oracle_lib, q[sel], v[sel], a[sel])
    W = pipe.W
    nl = g.robot().model.njoints - 1
    link_pos = getattr(pipe, "_link_pos", None)  # link-compact W: only the links with entries have a segment
    assert W.ld % 16 == 0 and W.cols == 16 * (nl if link_pos is None else int((link_pos >= 0).sum()))
    ref = np.arange(14 * nl)
    if link_pos is not None:
        dropped = link_pos[ref // 14] < 0
        assert not Wsel[:, dropped].any()  # what has no columns in W is identically zero in the oracle's regressor
        ref = ref[~dropped]
        pos = link_pos[ref // 14]
    else:
        pos = ref // 14
    dev_cols = pos * 16 + ref % 14
    ldf = getattr(W, "force_ld", 0)  # force-compact W: the force row blocks in a region of their own, in front
    nforce = (rps // 2) * N if ldf else 0
    tor = np.concatenate([j * N + sel for j in range(rps // 2 if ldf else 0, rps)])
    host = np.empty((len(tor), W.ld))
    base = W.buf.ptr + 8 * nforce * ldf
    for k, r in enumerate(tor):
        _lib.check(_lib.load().figh_memcpy_d2h(host[k].ctypes.data, base + int(r - nforce) * W.ld * 8, W.ld * 8))
    want = Wsel[(rps // 2) * len(sel):] if ldf else Wsel
    assert np.abs(host[:, dev_cols] - want[:, ref]).max() <= 1e-12 * np.abs(Wsel).max()
    pad = np.setdiff1d(np.arange(W.cols), dev_cols)
    assert not host[:, pad].any()
    if ldf:
        # force rows: mx my mz m of link p at columns 16 (p / 4) + 4 (p % 4) + (s - 6); the oracle's other entries are zeros
        frc = np.concatenate([j * N + sel for j in range(rps // 2)])
        hostf = np.empty((len(frc), ldf))
        for k, r in enumerate(frc):
            _lib.check(_lib.load().figh_memcpy_d2h(hostf[k].ctypes.data, W.buf.ptr + int(r) * ldf * 8, ldf * 8))
        wantf = Wsel[:(rps // 2) * len(sel)]
        fsl = (ref % 14 >= 6) & (ref % 14 <= 9)
        fcols = 16 * (pos[fsl] // 4) + 4 * (pos[fsl] % 4) + (ref[fsl] % 14 - 6)
        assert np.abs(hostf[:, fcols] - wantf[:, ref[fsl]]).max() <= 1e-12 * np.abs(Wsel).max()
        assert not wantf[:, ref[~fsl]].any()
        assert not hostf[:, np.setdiff1d(np.arange(ldf), fcols)].any()


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("layout", ["dense", "block-compact"])
def test_full_size_tiago_and_rank_crossing(lib, oracle_lib, layout):
    """BASELINE configs[2] (TIAGo, fv/fs/Ia/off, 1e6 samples = 24e6 x 336) at full size (examples/tiago/identification.py:293-337,
    qrdecomposition.py:208-221), plus the finding that comes with it: four structurally dependent pivots of the TIAGo
    regressor are genuine tiny numbers that grow like sqrt(N) (6.3e-9 at 1e5 samples, 1.26e-8 at 4e5) and cross
    TOL_QR = 1e-8, so the base-parameter count goes 179 -> 183 -> 185 with N -- in the REFERENCE too (np.linalg.qr of the same
    rows).  Checked from OUTSIDE the HIP path: against LAPACK on the oracle's W at 1e5 samples (all pivots, identical index
    set = the golden 179), against tests/golden/cfg3_tiago_large.json (oracle W + blocked LAPACK Householder TSQR,
    oracle/pin_cfg3_large.py) at 4e5 and at the BASELINE size 1e6.  ``dense`` is the link-padded resident W (spot rows
    against the oracle), ``block-compact`` the layout bench.py --config cfg3 runs."""
    from conftest import Golden
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    rng = np.random.default_rng(11)

    def tiago(N):
        g = Golden("cfg3_tiago")
        robot = g.robot()
        qva = sample_inputs(robot.model, N, np.random.default_rng(5), 1.5, 2, 5)
        pipe = IdentificationPipeline(robot, g.param, params_std=g.params_std(), coupling=g.coupling, w_layout=layout)
        pipe.set_samples(*qva)
        pipe.set_tau_from_parameters(g.phi_ref())
        return g, pipe, qva

    # (i) 1e5 samples: every |R_ii| against LAPACK on the oracle's matrix, base set = golden
    g, pipe, qva = tiago(100_000)
    out1 = pipe.run()
    assert out1["idx_e"] == list(g["idx_e"]) and out1["idx_base"] == list(g["idx_base"])
    assert out1["params_base"] == g.meta["params_base"]
    W_ref = _oracle_W(g, oracle_lib, *qva)
    keep = [i for i in range(W_ref.shape[1]) if i not in set(out1["idx_e"])]
    d_ref = np.abs(np.diag(np.linalg.qr(W_ref[:, keep], mode="r")))
    big = d_ref > 1e-8
    # phi against LAPACK on the same rows (north_star: 1e-6 relative): least squares of the oracle's base columns, from the
    # Householder triangle of [W_b tau] (np.linalg.qr) and one triangular solve
    from scipy.linalg import solve_triangular
    tau_host = pipe.d_tau.to_host()
    nb = int(big.sum())
    Rb = np.linalg.qr(np.c_[W_ref[:, np.asarray(keep)[big]], tau_host], mode="r")
    phi_lapack = solve_triangular(Rb[:nb, :nb], Rb[:nb, nb])
    assert np.abs(out1["phi_ls"] - phi_lapack).max() <= 1e-6 * np.abs(phi_lapack).max()
    del W_ref, Rb
    # (raw pivots of an UNPIVOTED QR are only comparable up to the direction of the noise reflectors of the dependent
    # columns in front of them -- SURVEY.md section 7 -- so: the decision exactly, the magnitudes loosely, and the four
    # borderline pivots, which carry the finding, tightly)
    assert [i for i in range(len(keep)) if big[i]] == out1["idx_base"]
    assert np.abs(out1["absdiagR"][big] / d_ref[big] - 1.0).max() <= 1e-3
    dep1 = np.sort(out1["absdiagR"][~big])[-4:]  # the four borderline pivots
    assert np.abs(np.sort(d_ref[~big])[-4:] / dep1 - 1.0).max() <= 1e-4 and dep1.min() > 3e-9
    del pipe
    # (ii) 4e5 samples: the same four pivots have doubled (sqrt(4)) and crossed the tolerance; pinned file
    with open(os.path.join(os.path.dirname(__file__), "golden", "cfg3_tiago_large.json")) as f:
        pinned = {(c["N"], c["seed"]): c for c in json.load(f)["cases"]}
    g, pipe, _ = tiago(400_000)
    out4 = pipe.run()
    pin4 = pinned[(400_000, 5)]
    assert out4["idx_e"] == pin4["idx_e"] == list(g["idx_e"]) and out4["idx_base"] == pin4["idx_base"]
    assert len(out4["idx_base"]) == 183
    for k, val in pin4["near_tolerance"].items():  # the pivots near TOL_QR themselves, on both sides of it
        assert abs(out4["absdiagR"][int(k)] / val - 1.0) <= 1e-4
    crossed = sorted(set(out4["idx_base"]) - set(out1["idx_base"]))
    assert len(crossed) == 4 and set(out1["idx_base"]) <= set(out4["idx_base"])
    ratio = np.sort(out4["absdiagR"][crossed]) / np.sort(dep1)
    assert np.all((ratio > 1.7) & (ratio < 2.3)), ratio
    del pipe
    # (iii) the BASELINE size
    g, pipe, qva = tiago(1_000_000)
    out = pipe.run()
    pin10 = pinned[(1_000_000, 5)]
    assert out["idx_e"] == pin10["idx_e"] == list(g["idx_e"]) and out["rows"] == 24_000_000
    assert out["idx_base"] == pin10["idx_base"] and len(out["idx_base"]) == 185  # (two more pivots have crossed)
    for k, val in pin10["near_tolerance"].items():
        assert abs(out["absdiagR"][int(k)] / val - 1.0) <= 1e-4
    assert out["absdiagR"][out["idx_base"]].min() > 1e-8
    kept = np.array([i for i in range(336) if i not in set(out["idx_e"])])
    assert np.abs(out["absdiagR"][0] ** 2 - out["col_norm"][kept[0]]) <= 1e-10 * out["col_norm"][kept[0]]  # R_00^2 = ||w_0||^2
    # phi_b reproduces the regrouped standard parameters of the 185-parameter base (tau = W phi_ref exactly): W_b phi = tau
    assert out["residual_norm"] <= 1e-6 * np.sqrt(out["rows"])
    if layout == "dense":
        _spot_rows_padded(pipe, g, oracle_lib, qva, 24, rng)
    else:
        assert pipe.W.compact is not None and pipe.W.buf.size * 8 < 12e9


@pytest.mark.timeout(900)
def test_full_size_talos(lib, oracle_lib):
    """BASELINE configs[3] (TALOS floating base, external wrench, 4e6 samples = 24e6 x 462) on one GPU: the structural
    results are the golden ones (produced by the reference's code at 32 / 400 samples), phi reproduces the regrouped
    standard parameters, and the triangle satisfies R^T R = W^T W on its diagonal (column norms from the fused K1' pass)."""
    rng = np.random.default_rng(12)
    g, pipe, qva = _tree_pipeline("cfg4_talos", 4_000_000, 5)
    out = pipe.run()
    assert out["idx_e"] == list(g["idx_e"]) and out["rows"] == 24_000_000
    assert out["idx_base"] == list(g["idx_base"]) and out["params_base"] == g.meta["params_base"]
    assert np.abs(out["phi_ls"] - g["phi_from_std"]).max() <= 1e-6 * np.abs(g["phi_from_std"]).max()
    dep = np.setdiff1d(np.arange(len(out["params_r"])), out["idx_base"])
    assert out["absdiagR"][dep].max() < 1e-8 < out["absdiagR"][out["idx_base"]].min()
    assert out["null_rule_certified"] and pipe.null_rule_fallbacks == 0
    _spot_rows_padded(pipe, g, oracle_lib, qva, 6, rng)


@pytest.mark.timeout(900)
def test_full_size_human_resident_link_compact(lib, oracle_lib):
    """BASELINE configs[4] at its stated size with W RESIDENT: the 21 massless links of the human model have no columns in
    the link-compact W (FIGH_FLAG_LINK_COMPACT: 19 x 16 = 304 instead of 640 columns, 146 GB for 6e7 rows), so 1e7 samples
    fit HBM in one piece -- golden idx_e / idx_base / expressions, phi to 1e-6, spot rows against the oracle."""
    rng = np.random.default_rng(13)
    g, pipe, qva = _tree_pipeline("cfg5_human", 10_000_000, 5)
    out = pipe.run()
    assert pipe._link_pos is not None and pipe.W.cols == 16 * 19
    assert out["idx_e"] == list(g["idx_e"]) and out["rows"] == 60_000_000
    assert out["idx_base"] == list(g["idx_base"]) and out["params_base"] == g.meta["params_base"]
    assert out["null_rule_certified"] and pipe.null_rule_fallbacks == 0
    assert np.abs(out["phi_ls"] - g["phi_from_std"]).max() <= 1e-6 * np.abs(g["phi_from_std"]).max()
    _spot_rows_padded(pipe, g, oracle_lib, qva, 6, rng)


@pytest.mark.parametrize("cfg", ["cfg5_human", "cfg4_talos"])
def test_force_compact_equals_one_matrix(lib, oracle_lib, cfg):
    """The force-compact W (force row blocks in their own region, one line per four links: FIGH_FLAG_FORCE_COMPACT, the default
    of the external-wrench regressor without friction columns) against the one-matrix form (w_layout="link-compact") on the
    same samples: column norms to 1e-13 (the force rows' squares are folded in another order), identical index sets and
    expressions, phi to 1e-9, every stored entry against the oracle; run(wls=True) re-creates W as one matrix and gives the
    one-matrix results."""
    from conftest import Golden
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    g = Golden(cfg)
    robot = g.robot()
    N = 20000 + 37
    rng = np.random.default_rng(9)
    qva = sample_inputs(robot.model, N, rng, 1.5, 2, 5)
    outs, pipes = [], []
    for layout in ("link-compact", "dense"):
        pipe = IdentificationPipeline(robot, g.param, params_std=g.params_std(), coupling=g.coupling, w_layout=layout)
        pipe.set_samples(*qva)
        pipe.set_tau_from_parameters(g.phi_ref(), noise_std=0.01, seed=2)
        pipe.run()
        outs.append(pipe.run())
        pipes.append(pipe)
    a_, b_ = outs
    nlive = int((pipes[1]._link_pos >= 0).sum()) if pipes[1]._link_pos is not None else robot.model.njoints - 1
    assert pipes[0]._force_ld == 0 and pipes[1]._force_ld == 16 * ((nlive + 3) // 4) == pipes[1].W.force_ld
    assert pipes[1].W.buf.size == 3 * N * (pipes[1]._force_ld + pipes[1].W.ld) < pipes[0].W.buf.size
    assert np.abs(a_["col_norm"] - b_["col_norm"]).max() <= 1e-13 * a_["col_norm"].max()
    assert a_["idx_e"] == b_["idx_e"] == list(g["idx_e"]) and a_["idx_base"] == b_["idx_base"] == list(g["idx_base"])
    assert a_["params_base"] == b_["params_base"] == g.meta["params_base"]
    assert np.abs(a_["phi_ls"] - b_["phi_ls"]).max() <= 1e-9 * np.abs(a_["phi_ls"]).max()
    assert abs(a_["residual_norm"] - b_["residual_norm"]) <= 1e-10 * a_["residual_norm"]
    _spot_rows_padded(pipes[1], g, oracle_lib, qva, 6, rng)
    _spot_rows_padded(pipes[0], g, oracle_lib, qva, 6, rng)
    with pytest.raises(ValueError):
        pipes[1].device_columns([6])
    w_ = pipes[1].run(wls=True)  # the weighted solve reads W as one matrix: the pipeline switches
    ref = pipes[0].run(wls=True)
    assert pipes[1]._force_ld == 0 and not hasattr(pipes[1].W, "force_ld")
    assert np.abs(w_["phi_wls"] - ref["phi_wls"]).max() <= 2e-6 and w_["idx_base"] == ref["idx_base"]


@pytest.mark.parametrize("cfg", ["cfg5_human", "cfg4_talos"])
def test_link_compact_equals_link_padded(lib, cfg):
    """The link-compact W of the external-wrench regressor against the link-padded one on the same samples: identical column
    norms (bit for bit: the same sums in the same order), index sets, expressions; phi to 1e-9; every stored segment
    identical, nothing stored for links without entries.  TALOS has no massless link: the layout must not engage."""
    from conftest import Golden
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    g = Golden(cfg)
    robot = g.robot()
    N = 20000 + 37
    q, v, a = sample_inputs(robot.model, N, np.random.default_rng(8), 1.5, 2, 5)
    outs, Ws, pipes = [], [], []
    for layout in ("link-padded", "dense"):
        pipe = IdentificationPipeline(robot, g.param, params_std=g.params_std(), coupling=g.coupling, w_layout=layout)
        pipe.set_samples(q, v, a)
        pipe.set_tau_from_parameters(g.phi_ref(), noise_std=0.01, seed=2)
        pipe.run()
        outs.append(pipe.run(wls=True))
        W = np.empty((pipe.W.rows, pipe.W.ld))
        lib.check(lib.load().figh_memcpy_d2h(W.ctypes.data, pipe.W.buf.ptr, W.nbytes))
        Ws.append(W)
        pipes.append(pipe)
    a_, b_ = outs
    nl = robot.model.njoints - 1
    if cfg == "cfg4_talos":
        assert pipes[1]._link_pos is None and Ws[1].shape == Ws[0].shape
    else:
        pos = pipes[1]._link_pos
        assert pos is not None and Ws[1].shape[1] == 16 * int((pos >= 0).sum()) < Ws[0].shape[1] == 16 * nl
        for l in range(nl):
            seg = Ws[0][:, 16 * l:16 * l + 16]
            if pos[l] < 0:
                assert not seg.any()
            else:
                assert np.array_equal(seg, Ws[1][:, 16 * pos[l]:16 * pos[l] + 16])
        with pytest.raises(ValueError):
            pipes[1].device_columns([14 * int(np.flatnonzero(pos < 0)[0])])
    assert np.array_equal(a_["col_norm"], b_["col_norm"])
    assert a_["idx_e"] == b_["idx_e"] == list(g["idx_e"]) and a_["idx_base"] == b_["idx_base"] == list(g["idx_base"])
    assert a_["params_base"] == b_["params_base"] == g.meta["params_base"]
    assert np.abs(a_["phi_ls"] - b_["phi_ls"]).max() <= 1e-9 * np.abs(a_["phi_ls"]).max()
    assert np.abs(a_["phi_wls"] - b_["phi_wls"]).max() <= 2e-6
    assert np.abs(a_["sigma2_joint"] - b_["sigma2_joint"]).max() <= 1e-9 * a_["sigma2_joint"].max()


@pytest.mark.timeout(900)
def test_full_size_human_streamed(lib):
    """BASELINE configs[4] (human whole body) streamed at its stated size, 1e7 samples (60e6 x 560 = 269 GB of W that never
    exists in full: chunks of 500 000 samples, norms-only first pass, link-padded chunk workspace): golden idx_e,
    idx_base and expressions, phi to 1e-6."""
    g, pipe, _ = _tree_pipeline("cfg5_human", 10_000_000, 5, chunk=500_000)
    out = pipe.run()
    assert out["idx_e"] == list(g["idx_e"]) and out["rows"] == 60_000_000
    assert out["idx_base"] == list(g["idx_base"]) and out["params_base"] == g.meta["params_base"]
    assert out["null_rule_certified"] and pipe.null_rule_fallbacks == 0
    assert np.abs(out["phi_ls"] - g["phi_from_std"]).max() <= 1e-6 * np.abs(g["phi_from_std"]).max()


def _parse_expression(e):
    """'Ixx5 - 1.0*Izz5 + 0.45*mz4' -> ('Ixx5', {'Izz5': -1.0, 'mz4': 0.45})"""
    tok = e.split(" ")
    terms = {}
    for sign, term in zip(tok[1::2], tok[2::2]):
        c, name = term.split("*")
        terms[name] = float(c) * (-1.0 if sign == "-" else 1.0)
    return tok[0], terms


def test_qr_pivoting_matches_reference(lib, golden, record_property):
    """QR_pivoting (qrdecomposition.py:24-86) through the TSQR triangle against the output of the reference's own
    function.  The reference's result is not a function of W_e alone: the pivot order among columns whose trailing
    norms tie (dependent families such as Ixx4 / Izz4 / Ia1 on the TX40, and the whole zero tail) is decided by the last
    bits -- LAPACK on W_e * (1 + 1e-15 noise) already returns another P (oracle/gen_golden_extra.py) -- so the check is
      - always: the rank, the shapes, the fitted torques W_b phi_b and the residual (invariant under the choice of
        base columns; tolerance = ||W_b|| * the 6-decimal rounding of phi), every expression a true regrouping
        (W_e[:, regrouped] = W_b beta to the rounding of beta), and the rank-0 result for a full-rank input (the
        reference's loop never reaches its else branch);
      - when the same base columns were picked: identical coefficients per base parameter and phi to the rounding."""
    import json
    from conftest import GOLD
    from figaroh_plus_amd.tools.qrdecomposition import QR_pivoting
    from figaroh_plus_amd.tools.regressor import build_regressor_reduced
    with open(os.path.join(GOLD, "qr_pivoting.json")) as f:
        gq = json.load(f)
    if golden.name not in gq:
        pytest.skip("no QR_pivoting fixture for this config")
    ref = gq[golden.name]
    g = golden
    W = _gpu_W(g, g["q_big"], g["v_big"], g["a_big"])
    W_e = build_regressor_reduced(W, list(g["idx_e"]))
    names = list(g.meta["params_r"])
    W_b, bp = QR_pivoting(g["tau"], W_e, names)
    r = len(ref["expressions"])
    assert len(bp) == r and list(W_b.shape) == ref["W_b_shape"]
    phi = np.array(list(bp.values()))
    parsed = [_parse_expression(e) for e in bp]
    base = [b for b, _ in parsed]
    assert len(set(base)) == r and np.array_equal(W_b, W_e[:, [names.index(b) for b in base]])
    # invariants of the fit
    tol = ref["W_b_colnorm_max"] * 0.5e-6 * r  # sum_j ||w_j|| |dphi_j|, |dphi_j| <= 0.5e-6
    pred = W_b @ phi
    assert abs(np.linalg.norm(pred) - ref["prediction_norm"]) <= 2 * tol
    assert abs(np.linalg.norm(g["tau"] - pred) - ref["residual_norm"]) <= 2 * tol
    # every expression is a regrouping: W_e[:, j] = sum_i beta_ij W_b[:, i] for the regrouped columns j
    regrouped = [n for n in names if n not in base]
    beta = np.zeros((r, len(regrouped)))
    for i, (_, terms) in enumerate(parsed):
        for n, c in terms.items():
            beta[i, regrouped.index(n)] = c
    err = np.abs(W_e[:, [names.index(n) for n in regrouped]] - W_b @ beta).max()
    assert err <= ref["W_b_colnorm_max"] * 1e-6 * r
    ref_parsed = dict(_parse_expression(e) for e in ref["expressions"])
    same_base = set(base) == set(ref_parsed)
    record_property("same_base_columns_as_reference", same_base)
    if golden.name == "cfg2_ur10":
        assert same_base  # the headline model has no tied trailing norms: the exact comparison below must have run
    if same_base:
        ref_phi = dict(zip((_parse_expression(e)[0] for e in ref["expressions"]), ref["phi_b"]))
        for (b, terms), x in zip(parsed, phi):
            assert terms == ref_parsed[b], b
            assert abs(x - ref_phi[b]) <= 1.5e-6, b
    W_b0, bp0 = QR_pivoting(g["tau"], W_e[:, g["idx_base"]], [names[i] for i in g["idx_base"]])
    assert list(W_b0.shape) == ref["full_rank_result"]["W_b_shape"] and len(bp0) == 0


# ------------------------------------------------------------------------------------------------ RCCL plumbing
def test_rccl_single_rank_roundtrip(lib):
    """The RCCL entry points on the one GPU a test box has: communicator of size 1, all-gather and all-reduce
    must return the input (validates the lazy dlopen, the symbol signatures and the stream the calls run on)."""
    import ctypes as C
    buf = C.create_string_buffer(128)
    l = lib.load()
    lib.check(l.figh_comm_available())  # the local preflight of dist.exchange_from_env
    lib.check(l.figh_comm_unique_id(buf))
    lib.check(l.figh_comm_init(1, 0, buf))
    try:
        x = np.arange(50 * 50, dtype=np.float64)
        d_x = lib.DeviceArray.from_host(x)
        d_all = lib.DeviceArray((x.size,))
        lib.check(l.figh_comm_allgather(d_x.ptr, d_all.ptr, x.size))
        assert np.array_equal(d_all.to_host(), x)
        lib.check(l.figh_comm_allreduce_sum(d_x.ptr, x.size))
        assert np.array_equal(d_x.to_host(), x)
        with pytest.raises(lib.FighError):
            lib.check(l.figh_comm_init(1, 0, buf))  # already initialised
    finally:
        lib.check(l.figh_comm_destroy())


def test_chunked_pipeline_equals_one_shot(lib, golden):
    """Memory-bounded mode (human model at 1e7 samples does not fit HBM as one W): two passes over sample chunks,
    triangles merged -- same structural result, same phi."""
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    g = golden
    N = len(g["q_big"])
    pipe = IdentificationPipeline(g.robot(), g.param, params_std=g.params_std(), coupling=g.coupling,
                                  chunk_samples=max(7, N // 3 + 1))
    pipe.set_samples(g["q_big"], g["v_big"], g["a_big"], g["tau"])
    out = pipe.run()
    assert out["idx_e"] == list(g["idx_e"])
    assert out["idx_base"] == list(g["idx_base"])
    assert out["params_base"] == g.meta["params_base"]
    assert np.abs(out["col_norm"] - g["colsq_big"]).max() <= 1e-12 * g["colsq_big"].max()
    assert np.abs(out["phi_ls"] - g["phi_pinv"]).max() <= 1e-6 * np.abs(g["phi_pinv"]).max()
    # second pass: ONE pass over the samples -- the kept set of the first pass is factored while the norms of all columns
    # come out of the same launches, and the set is verified afterwards (figh_regressor_tsqr_norms); same results
    chunked = pipe._chunked()  # (tile-blocked inputs round the chunk up to whole tiles: 32 TIAGo samples are one chunk)
    assert not chunked or pipe._chunk_kept is not None
    out2 = pipe.run()
    for key in ("idx_e", "idx_base", "params_base", "params_r"):
        assert out2[key] == out[key]
    assert np.abs(out2["col_norm"] - out["col_norm"]).max() <= 1e-13 * out["col_norm"].max()
    assert np.abs(out2["phi_ls"] - out["phi_ls"]).max() <= 1e-12 * np.abs(out["phi_ls"]).max()
    # a pass whose kept set differs from the cached one (another elimination threshold) notices and takes two passes
    kept_norms = np.sort(out["col_norm"][out["col_norm"] >= pipe.tol_e])
    if chunked and len(kept_norms) > 3 and kept_norms[0] < kept_norms[2]:
        pipe.tol_e = 0.5 * (kept_norms[0] + kept_norms[np.flatnonzero(kept_norms > kept_norms[0])[0]])  # drops the smallest
        out3 = pipe.run()
        assert len(out3["idx_e"]) > len(out["idx_e"]) and set(out["idx_e"]) < set(out3["idx_e"])
        assert len(out3["params_r"]) == len(out["params_r"]) - (len(out3["idx_e"]) - len(out["idx_e"]))
        out4 = pipe.run()  # and the new set is the cached one from then on
        assert out4["idx_e"] == out3["idx_e"] and out4["idx_base"] == out3["idx_base"]
        assert np.abs(out4["phi_ls"] - out3["phi_ls"]).max() <= 1e-12 * max(1.0, np.abs(out3["phi_ls"]).max())
    # synthetic tau built chunk by chunk equals W phi
    pipe2 = IdentificationPipeline(g.robot(), g.param, params_std=g.params_std(), coupling=g.coupling,
                                   chunk_samples=max(7, N // 3 + 1))
    pipe2.set_samples(g["q_big"], g["v_big"], g["a_big"])
    phi = g.phi_ref()
    tau = pipe2.set_tau_from_parameters(phi).to_host()
    W = _gpu_W(g, g["q_big"], g["v_big"], g["a_big"])
    assert np.abs(tau - W @ phi).max() <= 1e-11 * max(1.0, np.abs(W @ phi).max())


@pytest.mark.parametrize("cfg,model", [("cfg4_talos", "talos"), ("cfg5_human", "human")])
def test_wrench_force_rows_split(lib, cfg, model):
    """External wrench on a free-flyer root: (i) the rotational-inertia columns are EXACT zeros in the three force row
    blocks -- the assumption figh_tsqr_selected_wrench rests on; (ii) the pass that factors the force rows over the
    remaining columns only and chains the torque rows onto their triangle gives the results of the plain pass."""
    import json
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    from figaroh_plus_amd.tools.regressor import build_regressor_basic
    from figaroh_plus_amd.tools.robot import Robot
    root = os.path.dirname(__file__)
    meta = json.load(open(os.path.join(root, "golden", cfg + ".json")))
    robot = Robot.from_flat(model)
    rng = np.random.default_rng(11)
    q, v, a = sample_inputs(robot.model, 300, rng, 1.5, 2, 5)
    W = build_regressor_basic(robot, q, v, a, meta["param"])
    N = len(q)
    inertia = (np.arange(W.shape[1]) % 14) < 6
    assert not W[:3 * N][:, inertia].any()            # force rows: no dependence on the rotational inertia
    assert np.abs(W[3 * N:][:, inertia]).max() > 0.0  # torque rows do depend on it
    q, v, a = sample_inputs(robot.model, 6000, rng, 1.5, 2, 5)
    outs = []
    for split in (True, False):
        pipe = IdentificationPipeline(robot, meta["param"], params_std=dict(zip(meta["names_std"], meta["phi_ref_raw"])))
        pipe.set_samples(q, v, a)
        pipe.set_tau_from_parameters(np.array([float(x) for x in meta["phi_ref_raw"]]), noise_std=0.01, seed=3)
        out = pipe.run()
        if not split:
            pipe._wrench_split = False
            pipe._nf_expected = -1
            out = pipe.run()
        else:
            assert pipe._wrench_split and 0 < pipe._nf_expected < pipe._n_expected
            out = pipe.run()  # (a second pass: counts known from the start)
        outs.append(out)
    a_, b_ = outs
    assert a_["idx_e"] == b_["idx_e"] and a_["idx_base"] == b_["idx_base"] and a_["params_base"] == b_["params_base"]
    # |R_kk| is implementation independent up to the first dependent column only (behind it the reflector of a dependent
    # column points along rounding noise, see test_merge_base_rank_revealing_level); dependent pivots sit at roundoff
    n = len(a_["absdiagR"])
    rest = sorted(set(range(n)) - set(a_["idx_base"]))
    first_dep = rest[0] if rest else n
    assert np.abs(a_["absdiagR"] - b_["absdiagR"])[:first_dep].max() <= 1e-10 * b_["absdiagR"].max()
    assert a_["absdiagR"][rest].max(initial=0.0) <= 1e-9 * a_["absdiagR"].max()
    assert np.abs(a_["phi_ls"] - b_["phi_ls"]).max() <= 1e-8 * max(1.0, np.abs(b_["phi_ls"]).max())
    assert abs(a_["residual_norm"] - b_["residual_norm"]) <= 1e-9 * max(1.0, b_["residual_norm"])


@pytest.mark.parametrize("stride,with_tau,nlinks", [(16, True, 12), (14, False, 10), (16, False, 25)])
def test_structured_tsqr_entry_points_on_synthetic_matrices(lib, stride, with_tau, nlinks):
    """figh_tsqr_selected_wrench and figh_tsqr_selected_blocks at the C-ABI on random matrices that carry the structure
    (no model in the loop): R^T R of the plain triangle they return equals W_kept^T W_kept; with and without tau, both
    link strides, a block without any column, the fall-backs (too few rows / nf == n)."""
    rng = np.random.default_rng(stride * 100 + nlinks)
    ncols = 14 * nlinks
    ld = stride * nlinks
    # ---- six wrench row blocks: rotational-inertia columns zero in the force blocks; some all-zero (eliminated) columns
    Nb = 900
    rows = 6 * Nb
    Wref = rng.standard_normal((rows, ncols))
    dead = rng.choice(ncols, ncols // 5, replace=False)
    Wref[:, dead] = 0.0
    Wref[:3 * Nb][:, (np.arange(ncols) % 14) < 6] = 0.0
    tau = rng.standard_normal(rows)

    def to_device_layout(Wr):
        Wd = np.zeros((Wr.shape[0], ld))
        c = np.arange(ncols)
        Wd[:, (c // 14) * stride + c % 14] = Wr
        return Wd

    def run(entry, Wr, extra):
        Wd = to_device_layout(Wr)
        d_W = lib.DeviceArray.from_host(Wd.reshape(-1))
        d_cs = lib.DeviceArray.from_host((Wr ** 2).sum(axis=0))
        d_tau = lib.DeviceArray.from_host(tau[:Wr.shape[0]]) if with_tau else None
        d_sel = lib.DeviceArray((2 + 2 * ncols,), np.int32)
        kept = np.flatnonzero((Wr ** 2).sum(axis=0) >= 1e-6)
        n = len(kept)
        nc = n + (1 if with_tau else 0)
        d_R = lib.DeviceArray((nc * nc,))
        entry(d_W, Wr.shape[0], ld, d_cs, ncols, 1e-6, stride, n, *extra(kept), d_tau, -1.0, d_sel, d_R)
        sel = d_sel.to_host()
        assert sel[0] == n and np.array_equal(sel[2:2 + n], (kept // 14) * stride + kept % 14)
        R = d_R.to_host().reshape(nc, nc)
        A = Wr[:, kept] if not with_tau else np.c_[Wr[:, kept], tau[:Wr.shape[0]]]
        G = A.T @ A
        assert np.array_equal(R, np.triu(R))
        assert np.abs(R.T @ R - G).max() <= 1e-11 * np.abs(G).max()
        return kept

    if 14 * nlinks // 2 > 80:  # (the split needs the blocked kernel: more than 80 kept columns)
        run(lib.tsqr_selected_wrench, Wref, lambda kept: (int(np.count_nonzero(kept % 14 >= 6)),))
        run(lib.tsqr_selected_wrench, Wref, lambda kept: (0,))                      # nf unknown: plain path
        run(lib.tsqr_selected_wrench, Wref[:6 * 40], lambda kept: (int(np.count_nonzero(kept % 14 >= 6)),))  # too few rows
        # a STALE speculative count (the caller verifies it afterwards and discards the triangle): too large reads list
        # entries the split kernel never wrote, too small drops force columns -- neither may fault or leave the selection
        # wrong
        for delta in (+5, -3):
            d_W = lib.DeviceArray.from_host(to_device_layout(Wref).reshape(-1))
            d_cs = lib.DeviceArray.from_host((Wref ** 2).sum(axis=0))
            d_tau = lib.DeviceArray.from_host(tau) if with_tau else None
            d_sel = lib.DeviceArray((2 + 2 * ncols,), np.int32)
            kept = np.flatnonzero((Wref ** 2).sum(axis=0) >= 1e-6)
            n, nfk = len(kept), int(np.count_nonzero(kept % 14 >= 6))
            nc = n + (1 if with_tau else 0)
            d_R = lib.DeviceArray((nc * nc,))
            lib.tsqr_selected_wrench(d_W, rows, ld, d_cs, ncols, 1e-6, stride, n, nfk + delta, d_tau, -1.0, d_sel, d_R)
            lib.synchronize()
            sel = d_sel.to_host()
            assert sel[0] == n and np.array_equal(sel[2:2 + n], (kept // 14) * stride + kept % 14)
            assert np.all(np.isfinite(d_R.to_host()))
    # ---- nb row blocks with their own column subsets (one of them empty)
    nb = 7
    Nb2 = 700
    Wb = np.zeros((nb * Nb2, ncols))
    live = np.setdiff1d(np.arange(ncols), dead)
    subsets = []
    for j in range(nb):
        k = 0 if j == 3 else int(rng.integers(3, min(100, len(live))))
        sub = np.sort(rng.choice(live, k, replace=False))
        subsets.append(sub)
        Wb[j * Nb2:(j + 1) * Nb2][:, sub] = rng.standard_normal((Nb2, k))

    def block_args(kept):
        where = {c: i for i, c in enumerate(kept.tolist())}
        subs = [np.array([c for c in sub.tolist() if c in where], dtype=np.int64) for sub in subsets]
        counts = np.array([len(x) for x in subs], dtype=np.int32)
        cols = np.concatenate(subs + [np.zeros(1, dtype=np.int64)])
        pos = np.array([where[c] for x in subs for c in x.tolist()] + [0], dtype=np.int32)
        d_cols = lib.DeviceArray.from_host(((cols // 14) * stride + cols % 14).astype(np.int32))
        d_pos = lib.DeviceArray.from_host(pos)
        block_args.keep = (d_cols, d_pos)
        return counts, d_cols, d_pos

    run(lib.tsqr_selected_blocks, Wb, block_args)


def test_tree_row_blocks_column_lists(lib):
    """Joint-torque regressor of a tree (TIAGo): (i) row block j is exactly zero outside the columns the pipeline lists for
    it (subtree of joint j + own Ia / fv / fs / off) -- the assumption figh_tsqr_selected_blocks rests on; (ii) the pass
    that factors every row block over its own list gives the results of the plain pass."""
    import json
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    from figaroh_plus_amd.tools.regressor import build_regressor_basic
    from figaroh_plus_amd.tools.robot import Robot
    root = os.path.dirname(__file__)
    meta = json.load(open(os.path.join(root, "golden", "cfg3_tiago.json")))
    robot = Robot.from_flat("tiago")
    rng = np.random.default_rng(12)
    q, v, a = sample_inputs(robot.model, 3000, rng, 1.5, 2, 5)
    outs = []
    for blocks in (True, False):
        pipe = IdentificationPipeline(robot, meta["param"], params_std=dict(zip(meta["names_std"], meta["phi_ref_raw"])))
        pipe.set_samples(q, v, a)
        pipe.set_tau_from_parameters(np.array([float(x) for x in meta["phi_ref_raw"]]), noise_std=0.01, seed=3)
        out = pipe.run()
        if blocks:
            assert pipe._tree_blocks and pipe._block_cache is not None
            mask, counts, d_cols, d_pos = pipe._block_cache[:4]
            assert 0 < counts.max() < mask.sum() and counts.sum() < 0.3 * len(counts) * mask.sum()
            # the zero pattern of W against the lists (reference layout, a slice of the samples)
            W = build_regressor_basic(robot, q[:200], v[:200], a[:200], meta["param"])
            kept = np.flatnonzero(mask)
            pos = d_pos.to_host()
            off = 0
            for j, cnt in enumerate(counts):
                listed = np.zeros(len(kept), dtype=bool)
                listed[pos[off:off + cnt]] = True
                off += cnt
                blk = W[j * 200:(j + 1) * 200][:, kept]
                assert not blk[:, ~listed].any(), j
            out = pipe.run()
        else:
            pipe._tree_blocks = False
            out = pipe.run()
        outs.append(out)
    a_, b_ = outs
    assert a_["idx_e"] == b_["idx_e"] and a_["idx_base"] == b_["idx_base"] and a_["params_base"] == b_["params_base"]
    assert np.abs(a_["phi_ls"] - b_["phi_ls"]).max() <= 1e-8 * max(1.0, np.abs(b_["phi_ls"]).max())
    assert abs(a_["residual_norm"] - b_["residual_norm"]) <= 1e-9 * max(1.0, b_["residual_norm"])
    # (iii) block-compact W (FIGH_FLAG_COMPACT_BLOCKS): row block j stored as its own N x 16 |subtree_j| matrix; its content
    # is the window of the dense link-padded row, bit for bit, and the pass gives the dense pass's results exactly
    pipe_d = IdentificationPipeline(robot, meta["param"], params_std=dict(zip(meta["names_std"], meta["phi_ref_raw"])))
    pipe_c = IdentificationPipeline(robot, meta["param"], params_std=dict(zip(meta["names_std"], meta["phi_ref_raw"])),
                                    w_layout="block-compact")
    res = []
    for pipe in (pipe_d, pipe_c):
        pipe.set_samples(q, v, a)
        pipe.set_tau_from_parameters(np.array([float(x) for x in meta["phi_ref_raw"]]), noise_std=0.01, seed=3)
        pipe.run()
        res.append(pipe.run())
    assert pipe_c._compact is not None and pipe_d._compact is None
    N = len(q)
    dense = pipe_d.W.buf.to_host().reshape(pipe_d.W.rows, pipe_d.W.ld)
    comp = pipe_c.W.buf.to_host()
    off, ld = pipe_c._compact
    assert comp.size == N * ld.sum() and comp.size < 0.2 * dense.size
    for j in range(len(ld)):
        blk = comp[off[j]:off[j] + N * ld[j]].reshape(N, ld[j])
        assert np.array_equal(blk, dense[j * N:(j + 1) * N, 16 * j:16 * j + ld[j]]), j
        assert not dense[j * N:(j + 1) * N, :16 * j].any() and not dense[j * N:(j + 1) * N, 16 * j + ld[j]:].any()
    for key in ("idx_e", "idx_base", "params_base"):
        assert res[0][key] == res[1][key]
    assert np.array_equal(res[0]["phi_ls"], res[1]["phi_ls"]) and np.array_equal(res[0]["col_norm"], res[1]["col_norm"])


def test_structural_zeros_once_keeps_W_exact(lib):
    """Opt-in FIGH_FLAG_ZEROS_PRESENT (IdentificationPipeline(structural_zeros="once")): W is zero-filled once, the kernel
    rewrites the data-dependent entries only -- after repeated passes W equals the regressor the default kernel writes,
    bit for bit, and the results are those of the default pipeline."""
    import json
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    from figaroh_plus_amd.tools.robot import Robot
    root = os.path.dirname(__file__)
    meta = json.load(open(os.path.join(root, "golden", "cfg3_tiago.json")))
    robot = Robot.from_flat("tiago")
    rng = np.random.default_rng(13)
    sets = [sample_inputs(robot.model, 1500, rng, 1.5, 2, 5) for _ in range(2)]
    phi = np.array([float(x) for x in meta["phi_ref_raw"]])
    res = {}
    for mode in ("once", "every-pass"):
        pipe = IdentificationPipeline(robot, meta["param"], params_std=dict(zip(meta["names_std"], meta["phi_ref_raw"])),
                                      structural_zeros=mode)
        for q, v, a in sets:  # (set_samples allocates a fresh W: zero-filled again in "once" mode)
            pipe.set_samples(q, v, a)
            pipe.set_tau_from_parameters(phi, noise_std=0.01, seed=5)
            out = pipe.run()
            out = pipe.run()  # second pass into the same buffer
        assert getattr(pipe, "_zeros_once", False) == (mode == "once")
        res[mode] = (out, pipe.W.numpy().copy())
    assert np.array_equal(res["once"][1], res["every-pass"][1])
    a_, b_ = res["once"][0], res["every-pass"][0]
    assert a_["idx_e"] == b_["idx_e"] and a_["idx_base"] == b_["idx_base"] and a_["params_base"] == b_["params_base"]
    assert np.array_equal(a_["phi_ls"], b_["phi_ls"])


def test_tx40_real_data_known_answers_hip(lib):
    """Same known-answer replay with the HIP path end to end: Butterworth filtfilt of the joint positions on the
    device, K1 on the 44 958 real samples, two decimate-by-10 stages of every column of W and of tau on the device,
    then elimination, double_QR, sigma, OLS and WLS through the kernels; compared with the reference's committed
    TX40_bp_5.csv and with the reference-produced fixture (the filtered trajectories bit for bit)."""
    from tx40_real_common import decimate_and_filter, load_fixture, trajectories, tx40
    from figaroh_plus_amd.identification.identification_tools import (decimate_joint_blocks, least_squares,
                                                                       low_pass_filter_data, relative_stdev,
                                                                       weighted_least_squares_blocks)
    from figaroh_plus_amd.tools.qrdecomposition import double_QR
    from figaroh_plus_amd.tools.regressor import add_coupling_TX40, build_regressor_basic, eliminate_non_dynaffect
    z, meta = load_fixture()
    g, robot, param, params_std = tx40()
    q, dq, ddq, tau = trajectories(z, robot, param, low_pass_filter_data)
    sel = z["row_sel"]
    assert np.array_equal(q[sel], z["q_rows"]) and np.array_equal(dq[sel], z["dq_rows"])  # device filter == SciPy
    m = robot.model
    W = build_regressor_basic(robot, q, dq, ddq, param)
    W = add_coupling_TX40(W, m, robot.data, len(q), m.nq, m.nv, m.njoints, q, dq, ddq)
    chk = np.array([W.sum(), np.abs(W).sum(), (W * W).sum()])
    assert np.abs(chk - z["W_checksum"]).max() <= 1e-11 * np.abs(z["W_checksum"]).max()
    W_, tau_, counts = decimate_and_filter(W, tau, param, decimate_joint_blocks)
    assert counts == list(z["counts"])
    assert np.abs(W_[::97] - z["W_dec_rows"]).max() <= 1e-10 * np.abs(W_).max()
    W_e, params_r = eliminate_non_dynaffect(W_, params_std, 0.001)
    assert params_r == meta["params_r"]
    W_b, base_parameters, params_base, phi_b = double_QR(tau_, W_e, params_r)
    assert params_base == meta["csv_expressions"]
    csvv = z["csv"]
    assert np.abs(phi_b - z["phi_b"]).max() <= 1.5e-6
    assert np.abs(phi_b - csvv[:, 0]).max() <= 4e-4
    std = relative_stdev(W_b, phi_b, tau_)
    assert np.abs(std - z["std_ols"]).max() <= 0.011 + 1e-4 * np.abs(z["std_ols"]).max()
    assert (np.abs(std - csvv[:, 1]) / csvv[:, 1]).max() <= 0.012
    phi_ols = np.around(least_squares(W_b, tau_), 6)
    assert np.abs(phi_ols - z["phi_ols"]).max() <= 1.5e-6
    phi_w, std_w = weighted_least_squares_blocks(W_b, tau_, phi_b, counts)
    assert np.abs(phi_w - z["phi_wls"]).max() <= 1.5e-6
    assert np.abs(phi_w - csvv[:, 2]).max() <= 4e-4
    ok = z["std_wls"] < 1e3
    assert (np.abs(std_w - z["std_wls"])[ok] / z["std_wls"][ok]).max() <= 2e-3


@pytest.mark.parametrize("n", [1, 15, 16, 17, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 128, 193, 200, 257, 272, 305, 320, 330, 336, 384, 400,
                               511])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1000, 20011])
def test_tsqr_shapes_against_lapack(lib, n, rows):
    """Every kernel family / boundary of figh_tsqr (1 wave, tsqr2 4 and 5 chunks, every geometry of the blocked kernel
    incl. the two with a chunk in LDS: 321-336 and 385-400 columns with the tau column) on
    random full-rank matrices: R^T R = A^T A, |diag R| equals LAPACK's when rows >= n; tau column; row weights."""
    from figaroh_plus_amd.tools.qrdecomposition import rfactor
    rng = np.random.default_rng(1000 * n + rows)
    A = rng.standard_normal((rows, n)) * rng.uniform(0.5, 20.0, n)
    R = rfactor(A)
    assert R.shape == (n, n) and np.array_equal(R, np.triu(R))
    G = A.T @ A
    assert np.abs(R.T @ R - G).max() <= 1e-12 * np.abs(G).max()
    if rows >= n:
        ref = np.linalg.qr(A, mode="r")
        assert np.abs(np.abs(np.diag(R)) - np.abs(np.diag(ref))).max() <= 1e-9 * np.abs(np.diag(ref)).max()
    if rows >= n + 1 and rows % 7 == 0 or rows == 1000:
        t = rng.standard_normal(rows)
        w = rng.uniform(0.5, 2.0, 8 if rows % 8 == 0 else 1)
        Ra = rfactor(A, tau=t, block_weight=w)
        scale = np.repeat(w, rows // len(w))
        As = np.c_[A, t] * scale[:, None]
        Ga = As.T @ As
        assert np.abs(Ra.T @ Ra - Ga).max() <= 1e-12 * np.abs(Ga).max()


@pytest.mark.parametrize("n,rows", [(65, 850013), (72, 1000000), (79, 1000003), (80, 1250000)])
def test_tsqr_tall_65_to_80_columns_uses_the_48_row_form(lib, n, rows):
    """65 .. 80 columns and rows for eight waves per CU: level 0 runs as tsqr2_kernel<5, 3, false, true> (48-row tiles, last
    triangle chunk in registers, figh_linalg.hip) -- R^T R = A^T A, |diag R| equals LAPACK's, with and without tau, ragged
    last tile, gathered columns out of a wider matrix."""
    from figaroh_plus_amd.tools.qrdecomposition import rfactor
    rng = np.random.default_rng(n + rows)
    ld = n + 9
    W = rng.standard_normal((rows, ld)) * rng.uniform(0.5, 20.0, ld)
    cols = np.sort(rng.choice(ld, n - 1, replace=False)).astype(np.int32)
    t = rng.standard_normal(rows)
    A = np.c_[W[:, cols], t]
    G = A.T @ A
    R = rfactor(W, tau=t, col_idx=cols)
    assert R.shape == (n, n) and np.array_equal(R, np.triu(R))
    assert np.abs(R.T @ R - G).max() <= 1e-12 * np.abs(G).max()
    ref = np.linalg.qr(A[:200000], mode="r")  # (LAPACK on the whole matrix takes minutes: the Gram test above covers all rows)
    R2 = rfactor(W[:200000], tau=t[:200000], col_idx=cols)  # fewer rows: the 64-row form
    assert np.abs(np.abs(np.diag(R2)) - np.abs(np.diag(ref))).max() <= 1e-9 * np.abs(np.diag(ref)).max()
    Rn = rfactor(A[:, :n - 1] if n < 80 else A)  # no tau / all columns
    Gn = G[:Rn.shape[0], :Rn.shape[0]]
    assert np.abs(Rn.T @ Rn - Gn).max() <= 1e-12 * np.abs(Gn).max()


def _rank_deficient(rng, rows, n, ndep):
    """rows x n, ndep of the columns (at random places, never the first) exact combinations of columns in front of them"""
    A = rng.standard_normal((rows, n)) * rng.uniform(0.5, 20.0, n)
    dep = np.sort(rng.choice(np.arange(1, n), ndep, replace=False))
    for j in dep:
        src = [k for k in range(j) if k not in set(dep.tolist())]
        pick = rng.choice(src, min(3, len(src)), replace=False)
        A[:, j] = A[:, pick] @ rng.uniform(-2.0, 2.0, len(pick))
    return A, dep


@pytest.mark.parametrize("n,ndep", [(50, 13), (64, 20), (80, 9), (96, 30), (191, 27), (241, 60), (331, 96), (400, 40)])
@pytest.mark.parametrize("rows", [4096, 50011])
def test_null_pivot_rule_on_rank_deficient_matrices(lib, n, ndep, rows):
    """figh_tsqr_null_pivot_tol (include/figh.h): dependent columns -- qrdecomposition.py:208-221's |R_kk| <= tol_qr -- skip
    their column steps.  Every kernel family.  With and without the rule: the same base set, R^T R = A^T A to rounding,
    |R_kk| of the dependent columns below tol_qr and equal in size, the base solution identical."""
    from figaroh_plus_amd import _lib
    from figaroh_plus_amd.tools.qrdecomposition import rfactor
    rng = np.random.default_rng(77 * n + rows)
    A, dep = _rank_deficient(rng, rows, n, ndep)
    t = A @ rng.standard_normal(n) + 0.1 * rng.standard_normal(rows)
    G = np.c_[A, t].T @ np.c_[A, t]
    out = {}
    try:
        for tol in (0.0, 1e-8 / 64):
            _lib.tsqr_null_pivot_tol(tol)
            out[tol] = rfactor(A, tau=t)
    finally:
        _lib.tsqr_null_pivot_tol(0.0)
    base = np.setdiff1d(np.arange(n), dep)
    phi = {}
    for tol, R in out.items():
        assert np.array_equal(R, np.triu(R))
        assert np.abs(R.T @ R - G).max() <= 1e-12 * np.abs(G).max()
        d = np.abs(np.diag(R))[:n]
        assert np.array_equal(np.flatnonzero(d > 1e-8), base)
        assert d[dep].max() <= 5e-9
        Rb = np.linalg.qr(R[:, list(base) + [n]], mode="r")
        phi[tol] = np.linalg.solve(Rb[:len(base), :len(base)], Rb[:len(base), -1])
    assert np.abs(phi[0.0] - phi[1e-8 / 64]).max() <= 1e-10 * np.abs(phi[0.0]).max()
    ref = np.linalg.lstsq(A[:, base], t, rcond=None)[0]
    assert np.abs(phi[1e-8 / 64] - ref).max() <= 1e-9 * np.abs(ref).max()


@pytest.mark.parametrize("n", [50, 96, 241, 331])
def test_null_pivot_rule_column_that_becomes_independent_late(lib, n):
    """A column that is an exact combination of earlier ones in the first 90 % of the rows and not in the rest (a joint that
    only starts to move late in the trajectory): null in the early tiles, a regular pivot from the first tile in which it
    is not.  Nothing of it may be lost: R^T R = A^T A, the column is a base column, same solution as LAPACK."""
    from figaroh_plus_amd import _lib
    from figaroh_plus_amd.tools.qrdecomposition import rfactor
    rows = 40000
    rng = np.random.default_rng(5 * n)
    A, dep = _rank_deficient(rng, rows, n, max(3, n // 6))
    late = int(dep[len(dep) // 2])
    A[36000:, late] += rng.standard_normal(rows - 36000)
    tiny = int(dep[0])                      # ... and one that differs from its combination by 1e-10 per entry throughout:
    A[:, tiny] += 1e-10 * rng.standard_normal(rows)   # |R_kk| ~ 2e-8 > tol_qr, folded in no tile but the first few
    t = A @ rng.standard_normal(n) + 0.1 * rng.standard_normal(rows)
    G = np.c_[A, t].T @ np.c_[A, t]
    try:
        _lib.tsqr_null_pivot_tol(1e-8 / 64)
        R = rfactor(A, tau=t)
        _lib.tsqr_null_pivot_tol(0.0)
        R0 = rfactor(A, tau=t)
    finally:
        _lib.tsqr_null_pivot_tol(0.0)
    assert np.abs(R.T @ R - G).max() <= 1e-12 * np.abs(G).max()
    d, d0 = np.abs(np.diag(R))[:n], np.abs(np.diag(R0))[:n]
    base = np.flatnonzero(d > 1e-8)
    assert np.array_equal(base, np.flatnonzero(d0 > 1e-8))
    assert late in base and tiny in base and len(base) == n - len(dep) + 2
    assert abs(d[tiny] - d0[tiny]) <= 0.02 * d0[tiny]
    ref = np.linalg.lstsq(A[:, np.setdiff1d(base, [tiny])], t, rcond=None)[0]
    keep = [int(k) for k in base if k != tiny]
    Rb = np.linalg.qr(R[:, keep + [n]], mode="r")
    phi = np.linalg.solve(Rb[:len(keep), :len(keep)], Rb[:len(keep), -1])
    assert np.abs(phi - ref).max() <= 1e-7 * np.abs(ref).max()


def test_regressor_leading_dimension_and_colsq(lib, golden_ur10):
    """ldw > ncols (padded rows, scalar store path) and the fused column norms against figh_colsq."""
    from figaroh_plus_amd import _lib
    from figaroh_plus_amd.tools.regressor import regressor_flags
    g = golden_ur10
    robot = g.robot()
    q, v, a = g["q_big"], g["v_big"], g["a_big"]
    N, ldw = len(q), 91
    dq, dv, da = (_lib.DeviceArray.from_host(np.ascontiguousarray(x).reshape(-1)) for x in (q, v, a))
    dW = _lib.DeviceArray.from_host(np.full(6 * N * ldw, -7.0))
    dcs = _lib.DeviceArray((84,))
    mode, flags, ft = regressor_flags(g.param)
    _lib.regressor_build(robot.device_model(), mode, flags, ft, N, dq, dv, da, dW, ldw, dcs)
    Wp = dW.to_host().reshape(6 * N, ldw)
    assert np.all(Wp[:, 84:] == -7.0)                       # padding untouched
    ref = _gpu_W(g, q, v, a)
    assert np.array_equal(Wp[:, :84], ref)
    cs = dcs.to_host()
    d2 = _lib.DeviceArray((84,))
    _lib.colsq(dW, 6 * N, 84, ldw, d2)
    assert np.abs(cs - d2.to_host()).max() <= 1e-13 * cs.max()
    with pytest.raises(_lib.FighError):
        _lib.regressor_build(robot.device_model(), mode, flags, ft, N, dq, dv, da, dW, 80, None)  # ldw < ncols


# ------------------------------------------------------------------------------------------------ streamed C-ABI
@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [0, 64, 150])
def test_streamed_entry_points_equal_materialised(lib, golden, chunk):
    """figh_regressor_colsq / figh_regressor_tsqr / figh_regressor_gram (W never stored in full, SURVEY 8b 'fused'
    forms) against the same quantities of the materialised W: column norms, R^T R = W_e^T W_e, W_e^T tau, tau^T tau,
    the rank decision and a joint-weighted variant."""
    from figaroh_plus_amd import _lib
    from figaroh_plus_amd.tools.regressor import regressor_flags
    g = golden
    q, v, a, tau = g["q_big"], g["v_big"], g["a_big"], g["tau"]
    N = len(q)
    W = _gpu_W(g, q, v, a)
    robot = g.robot()
    dm = robot.device_model()
    mode, flags, ft = regressor_flags(g.param, g.coupling)
    rps, ncols = dm.shape(mode, flags)
    assert W.shape == (rps * N, ncols)
    d_q, d_v, d_a = (_lib.DeviceArray.from_host(np.ascontiguousarray(x).reshape(-1)) for x in (q, v, a))
    d_c = _lib.DeviceArray((ncols,))
    _lib.regressor_colsq(dm, mode, flags, ft, N, d_q, d_v, d_a, d_c, chunk_samples=chunk)
    ref_c = np.einsum("ij,ij->j", W, W)
    assert np.abs(d_c.to_host() - ref_c).max() <= 1e-12 * ref_c.max()
    keep = [i for i in range(ncols) if i not in set(g["idx_e"].tolist())]
    n = len(keep)
    d_idx = _lib.DeviceArray.from_host(np.asarray(keep, dtype=np.int32))
    d_tau = _lib.DeviceArray.from_host(tau)
    d_R = _lib.DeviceArray(((n + 1) * (n + 1),))
    _lib.regressor_tsqr(dm, mode, flags, ft, N, d_q, d_v, d_a, d_idx, n, d_tau, None, d_R, chunk_samples=chunk)
    R = np.triu(d_R.to_host().reshape(n + 1, n + 1))
    We = W[:, keep]
    A = np.c_[We, tau]
    G = A.T @ A
    assert np.abs(R.T @ R - G).max() <= 1e-11 * np.abs(G).max()
    d = np.abs(np.diag(R))[:n]
    assert [i for i in range(n) if d[i] > 1e-8] == list(g["idx_base"])
    Gs, gs, tt = _lib.regressor_gram(dm, mode, flags, ft, N, d_q, d_v, d_a, d_idx, n, d_tau, chunk_samples=chunk)
    assert np.abs(Gs - G[:n, :n]).max() <= 1e-11 * np.abs(G).max()
    assert np.abs(gs - G[:n, n]).max() <= 1e-11 * np.abs(G[:n, n]).max()
    assert abs(tt - G[n, n]) <= 1e-11 * G[n, n]
    # one weight per row of a sample (joint / wrench component): QR of the row-scaled matrix
    w = 0.5 + np.arange(rps) / rps
    _lib.regressor_tsqr(dm, mode, flags, ft, N, d_q, d_v, d_a, d_idx, n, d_tau, w, d_R, chunk_samples=chunk)
    Rw = np.triu(d_R.to_host().reshape(n + 1, n + 1))
    Aw = A * np.repeat(w, N)[:, None]
    Gw = Aw.T @ Aw
    assert np.abs(Rw.T @ Rw - Gw).max() <= 1e-11 * np.abs(Gw).max()


# ------------------------------------------------------------------------------------------------ 8f-1 preprocessing
@pytest.mark.parametrize("L,cols,nblocks,q", [(28, 1, 1, 10), (100, 3, 2, 10), (4496, 7, 6, 10), (1001, 5, 3, 4), (300, 2, 1, 1)])
def test_decimate_matches_scipy(lib, L, cols, nblocks, q):
    """figh_filtfilt_cols against scipy.signal.decimate(zero_phase=True) / sosfiltfilt, sequence by sequence: the
    recurrences are SciPy's operation by operation, so the agreement is at rounding level (bit-equal in practice)."""
    from scipy import signal
    from figaroh_plus_amd.identification.identification_tools import _decimate_design, _filtfilt_device
    rng = np.random.default_rng(L + cols)
    t = np.arange(L * nblocks)[:, None]
    x = np.sin(0.01 * t * (1 + np.arange(cols))) + 0.1 * rng.standard_normal((L * nblocks, cols)) + 3.0
    sos, zi, padlen = _decimate_design(max(q, 2))
    y = _filtfilt_device(x, nblocks, 0, sos[:, :3], sos[:, 3:], zi, padlen, q)
    ref = np.vstack([signal.sosfiltfilt(sos, x[b * L:(b + 1) * L], axis=0)[::q] for b in range(nblocks)])
    assert y.shape == ref.shape
    assert np.abs(y - ref).max() <= 1e-13 * np.abs(ref).max()
    if q >= 2:
        ref2 = np.vstack([signal.decimate(x[b * L:(b + 1) * L], q, zero_phase=True, axis=0) for b in range(nblocks)])
        assert np.abs(y - ref2).max() <= 1e-13 * np.abs(ref2).max()


def test_filtfilt_tf_matches_scipy_and_errors(lib):
    from scipy import signal
    from figaroh_plus_amd import _lib
    from figaroh_plus_amd.identification.identification_tools import (_filtfilt_device, decimate_joint_blocks,
                                                                       low_pass_filter_data)
    rng = np.random.default_rng(3)
    x = np.cumsum(rng.standard_normal((5000, 4)), axis=0)
    param = {"ts": 0.0002, "cut_off_frequency_butterworth": 100.0}
    for nb in (4, 5):
        got = low_pass_filter_data(x, param, nb)
        b, a = signal.butter(nb, param["ts"] * param["cut_off_frequency_butterworth"] / 2, "low")
        ref = signal.filtfilt(b, a, x, axis=0, padtype="odd", padlen=3 * (max(len(b), len(a)) - 1))[5 * nb:-5 * nb]
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    one = low_pass_filter_data(x[:, 0], param, 4)  # 1-D input like the reference's per-joint call
    assert one.shape == (5000 - 40,)
    with pytest.raises(ValueError):  # SciPy: "The length of the input vector x must be greater than padlen"
        decimate_joint_blocks(np.ones((27 * 2, 3)), np.ones(27 * 2), 2)
    with pytest.raises(_lib.FighError):
        _filtfilt_device(np.ones((20, 1)), 1, 1, np.ones(3), np.ones(3), np.ones(2), 30, 1)


# ------------------------------------------------------------------------------------------------ 8f-2 objective
def test_excitation_objective_matches_numpy_cond(lib, golden, oracle_lib):
    """cond(W_b) of examples/tiago/optimal_trajectory.py:100-133 without storing W: streamed triangle, optional stack."""
    from figaroh_plus_amd.tools.excitation import base_regressor_triangle, objective_cond
    g = golden
    q, v, a = g["q_big"], g["v_big"], g["a_big"]
    W = _oracle_W(g, oracle_lib, q, v, a)  # the reference side never touches the HIP kernels
    keep = [i for i in range(W.shape[1]) if i not in set(g["idx_e"].tolist())]
    Wb = W[:, keep][:, g["idx_base"]]
    ref = np.linalg.cond(Wb)
    got = objective_cond(g.robot(), q, v, a, g.param, g["idx_e"], g["idx_base"], coupling=g.coupling)
    assert abs(got - ref) <= 1e-9 * ref
    # second trajectory stacked under the first: cond(vstack) from the merged triangles
    h = len(q) // 2
    R1 = base_regressor_triangle(g.robot(), q[:h], v[:h], a[:h], g.param, g["idx_e"], g["idx_base"], coupling=g.coupling)
    got2 = objective_cond(g.robot(), q[h:], v[h:], a[h:], g.param, g["idx_e"], g["idx_base"], R_stack=R1,
                          coupling=g.coupling)
    assert abs(got2 - ref) <= 1e-9 * ref  # same rows as the one-shot matrix, stacked in two pieces


@pytest.mark.parametrize("n_per,B,stacked", [(130, 3, False), (130, 3, True), (1000, 4, False), (64, 7, True)])
def test_excitation_objective_batch_matches_numpy_cond(lib, golden, oracle_lib, n_per, B, stacked):
    """objective_cond_batch: B trajectories of one finite-difference gradient (optimal_trajectory.py:296-313) in one K1
    launch + one batched TSQR launch (more than 80 base columns; trajectory by trajectory otherwise), against
    np.linalg.cond of every trajectory's materialised W_b -- alone and stacked under a previous regressor.  n_per is not a
    multiple of the tile height: the ragged end of every row segment is followed by the next trajectory's rows."""
    from figaroh_plus_amd.tools.excitation import base_regressor_triangle, objective_cond, objective_cond_batch
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    g = golden
    robot = g.robot()
    rng = np.random.default_rng(n_per + B)
    trajs = [sample_inputs(robot.model, n_per, rng, 1.5, 2, 5) for _ in range(B)]
    gone = set(g["idx_e"].tolist())
    R_stack, W_stack = None, None
    if stacked:
        qs, vs, as_ = sample_inputs(robot.model, 200, rng, 1.5, 2, 5)
        W = _oracle_W(g, oracle_lib, qs, vs, as_)
        keep = [i for i in range(W.shape[1]) if i not in gone]
        W_stack = W[:, keep][:, g["idx_base"]]
        R_stack = base_regressor_triangle(robot, qs, vs, as_, g.param, g["idx_e"], g["idx_base"], coupling=g.coupling)
    got = objective_cond_batch(robot, trajs, g.param, g["idx_e"], g["idx_base"], R_stack=R_stack, coupling=g.coupling)
    assert len(got) == B
    for b, (q, v, a) in enumerate(trajs):
        W = _oracle_W(g, oracle_lib, q, v, a)  # the reference side never touches the HIP kernels
        keep = [i for i in range(W.shape[1]) if i not in gone]
        Wb = W[:, keep][:, g["idx_base"]]
        if stacked:
            Wb = np.vstack((W_stack, Wb))
        ref = np.linalg.cond(Wb)
        assert abs(got[b] - ref) <= 1e-9 * ref, (b, got[b], ref)
        if b == 0:  # and the one-trajectory entry point agrees
            one = objective_cond(robot, q, v, a, g.param, g["idx_e"], g["idx_base"], R_stack=R_stack, coupling=g.coupling)
            assert abs(one - got[0]) <= 1e-9 * ref
    with pytest.raises(ValueError):
        objective_cond_batch(robot, [trajs[0], tuple(x[:-1] for x in trajs[0])], g.param, g["idx_e"], g["idx_base"],
                             coupling=g.coupling)


# ------------------------------------------------------------------------------------------------ 8f-3 SIP QP terms
def test_sip_qp_terms_match_reference_formulas(lib, golden, oracle_lib):
    """P and r of calculate_standard_parameters (identification_tools.py:528-531) against the same NumPy statements on
    the materialised W (inertial columns only, as the human example passes them)."""
    from figaroh_plus_amd.identification.identification_tools import sip_qp_terms
    g = golden
    q, v, a, tau = g["q_big"], g["v_big"], g["a_big"], g["tau"]
    W = _oracle_W(g, oracle_lib, q, v, a)  # the reference side never touches the HIP kernels
    nl = (W.shape[1] - (3 if g.coupling else 0)) // 14
    cols = [14 * k + s for k in range(nl) for s in range(10)]
    phi_ref = np.linspace(0.5, 2.0, len(cols))
    alpha = 0.8
    P, r = sip_qp_terms(g.robot(), q, v, a, tau, g.param, cols, phi_ref, alpha, coupling=g.coupling)
    Wc = W[:, cols]
    sf1 = 1 / (np.max(phi_ref) * len(phi_ref))
    sf2 = 1 / (np.max(tau) * len(tau))
    P_ref = (1 - alpha) * sf1 * np.eye(Wc.shape[1]) + alpha * sf2 * np.matmul(Wc.T, Wc)
    r_ref = -((1 - alpha) * sf1 * phi_ref.T + sf2 * alpha * np.matmul(tau.T, Wc))
    assert np.abs(P - P_ref).max() <= 1e-11 * np.abs(P_ref).max()
    assert np.abs(r - r_ref).max() <= 1e-11 * np.abs(r_ref).max()


def test_calculate_standard_parameters_matches_reference(lib, golden):
    """calculate_standard_parameters (identification_tools.py:466-572) end to end: W of the inertial columns built and
    reduced on the device, the program solved on the host, against the reference's own function (fixture
    tests/golden/sip_qp.npz: its quadprog arguments and the solution of that program, oracle/gen_golden_extra.py)."""
    from figaroh_plus_amd.identification import identification_tools as idt
    g = golden
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "sip_qp.npz"))
    if g.name + "/cols" not in z.files:
        # fixed-base models (TX40, UR10, TIAGo): the base link is welded to the universe, whose inertia then has mass
        # (4.2 / 204 / 42.85 kg), so id_inertias starts at joint 0 and the reference looks up 'Ixx0', which
        # get_standard_parameters never writes (identification_tools.py:497-514, robot.py:102-119) -- KeyError there and here.
        # (The reference's function only ever runs on the floating-base models: examples/human/identification.py.)
        model = g.robot().model
        assert model.inertias[0].mass != 0 and g.name in ("cfg1_tx40", "cfg2_ur10", "cfg3_tiago")
        nreal = sum(1 for i in model.inertias.tolist() if i.mass != 0)
        W = _gpu_W(g, g["q_big"][:64], g["v_big"][:64], g["a_big"][:64])
        cols = [14 * k + s for k in range(model.njoints - 1) for s in range(10)]
        with pytest.raises(KeyError, match="Ixx0"):
            idt.calculate_standard_parameters(model, W[:, cols], np.ones(len(W)), np.ones(3 * nreal), -np.ones(3 * nreal),
                                              g.params_std(), 0.33)
        return
    f = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(g.name + "/")}
    W = _gpu_W(g, g["q_big"], g["v_big"], g["a_big"])
    Wc = np.ascontiguousarray(W[:, f["cols"]])
    seen = {}
    real = idt.quadprog_solve_qp

    def spy(P, q, G=None, h=None, A=None, b=None):
        seen.update(P=P, q=q)
        return real(P, q, G, h, A, b)

    idt.quadprog_solve_qp = spy
    try:
        phi, phi_ref = idt.calculate_standard_parameters(g.robot().model, Wc, g["tau"], f["COM_max"], f["COM_min"],
                                                         g.params_std(), float(f["alpha"]))
    finally:
        idt.quadprog_solve_qp = real
    assert np.array_equal(phi_ref, f["phi_ref"])
    n = len(phi)
    qp_G = 0.5 * (seen["P"] + seen["P"].T) + 1e-5 * np.eye(n)
    assert np.abs(qp_G - f["qp_G"]).max() <= 1e-11 * np.abs(f["qp_G"]).max()
    assert np.abs(-seen["q"] - f["qp_a"]).max() <= 1e-11 * np.abs(f["qp_a"]).max()
    assert np.abs(phi - f["phi_standard"]).max() <= 1e-8 * np.abs(f["phi_standard"]).max()
    with pytest.raises(ValueError):
        idt.calculate_standard_parameters(g.robot().model, Wc[:, :-1], g["tau"], f["COM_max"], f["COM_min"],
                                          g.params_std(), 0.33)


# ------------------------------------------------------------------------------------------------ 8f-4 TLS payload
def _tls_check(out, ref, pre, W_tot_rows):
    W_tot, V_norm, residue = out
    assert list(W_tot.shape) == ref[pre + "shape"].tolist()
    cs = ref[pre + "checksum"]
    assert abs(W_tot.sum() - cs[0]) <= 1e-10 * cs[1] and abs(np.abs(W_tot).sum() - cs[1]) <= 1e-11 * cs[1]
    # the singular vector of the smallest singular value: conditioned by the gap to the next one (fixture: 3 % - 30x)
    assert np.abs(V_norm - ref[pre + "V_norm"]).max() <= 1e-8 * np.abs(ref[pre + "V_norm"]).max()
    assert np.abs(residue - ref[pre + "residue"]).max() <= 1e-8 * np.abs(ref[pre + "residue"]).max()


def test_total_regressor_current_matches_reference(lib, golden_tx40, oracle_lib):
    """build_total_regressor_current (regressor.py:296-412) against the output of the reference's own function
    (tests/golden/tls_regressors.npz, oracle/gen_golden_extra.py) in its three column layouts; W_tot assembled on the
    device, TLS vector from the SVD of its TSQR triangle, residue by a device mat-vec."""
    from figaroh_plus_amd.device import GpuMatrix
    from figaroh_plus_amd.tools.regressor import build_total_regressor_current
    g = golden_tx40
    ref = np.load(os.path.join(os.path.dirname(__file__), "golden", "tls_regressors.npz"))
    W = _gpu_W(g, g["q_big"], g["v_big"], g["a_big"])
    half, rows_u, rows_l, W_b_u, W_b_l, W_l = oracle_np.tls_inputs(W, g.z, 6)
    I_u, I_l = ref["current/I_u"], ref["current/I_l"]
    for name, fr, ia in (("friction", True, True), ("actuator", False, True), ("plain", False, False)):
        param = dict(g.param, has_friction=fr, has_actuator_inertia=ia, nb_samples=half, which_body_loaded=5, mass_load=3.0)
        out = build_total_regressor_current(W_b_u, W_b_l, W_l, I_u, I_l, g.params_std(), param)
        _tls_check(out, ref, "current/%s/" % name, 2 * len(W_l))
    # device-resident inputs stay on the device
    out = build_total_regressor_current(GpuMatrix.from_host(W_b_u), W_b_l, W_l, I_u, I_l, g.params_std(), param)
    assert isinstance(out[0], GpuMatrix)
    _tls_check((out[0].numpy(), out[1], out[2]), ref, "current/plain/", 2 * len(W_l))
    # the reference's np.concatenate failures
    with pytest.raises(ValueError):
        build_total_regressor_current(W_b_u[:-1], W_b_l, W_l, I_u, I_l, g.params_std(), param)
    with pytest.raises(ValueError):
        build_total_regressor_current(W_b_u, W_b_l[:, :-1], W_l, I_u, I_l, g.params_std(), param)
    with pytest.raises(IndexError):
        build_total_regressor_current(W_b_u, W_b_l, W_l, I_u, I_l, g.params_std(), dict(param, which_body_loaded=9))


def test_total_regressor_wrench_matches_reference(lib):
    """build_total_regressor_wrench (regressor.py:415-500) on the human model, same fixture."""
    from conftest import Golden
    from figaroh_plus_amd.tools.regressor import build_total_regressor_wrench
    g = Golden("cfg5_human")
    ref = np.load(os.path.join(os.path.dirname(__file__), "golden", "tls_regressors.npz"))
    W = _gpu_W(g, g["q_big"], g["v_big"], g["a_big"])
    half, rows_u, rows_l, W_b_u, W_b_l, W_l = oracle_np.tls_inputs(W, g.z, 6, nbase=40)
    W_l = np.ascontiguousarray(W_l[:, [14 * k + s for k in range(W.shape[1] // 14) for s in range(10)]])
    param = dict(g.param, which_body_loaded=int(ref["wrench/body"]), mass_load=2.0)
    out = build_total_regressor_wrench(W_b_u, W_b_l, W_l, ref["wrench/tau_u"], ref["wrench/tau_l"], g.params_std(), param)
    _tls_check(out, ref, "wrench/", 2 * len(W_l))


@pytest.mark.parametrize("case", ["tx40_full", "tx40_full_noq", "talos_offsets"])
def test_calibration_base_regressor_matches_reference(lib, case, capsys):
    """calculate_base_kinematics_regressor (calibration_tools.py:1469-1561), the second caller of the elimination /
    base-parameter functions, against the output of the reference's own function (fixture
    tests/golden/calibration_base_regressor.json, oracle/gen_golden_extra.py; the calibration subsystem's kinematic
    regressor is the same synthetic stand-in on both sides): names, expressions, shapes, matrices, the side effect on
    param["param_name"] and the printed shapes."""
    import json
    from figaroh_plus_amd.calibration.calibration_tools import calculate_base_kinematics_regressor
    from figaroh_plus_amd.tools.robot import Robot
    with open(os.path.join(os.path.dirname(__file__), "golden", "calibration_base_regressor.json")) as f:
        ref = json.load(f)[case]
    model = Robot.from_flat(ref["model"]).model
    q = np.array(ref["q"])
    param = {"free_flyer": ref["free_flyer"], "calib_model": ref["calib_model"], "param_name": ["pre-existing"]}
    ncols = 6 * (model.njoints - 1) if ref["calib_model"] == "full_params" else model.nv
    calls = []

    def kin(q_, model_, data_, param_):
        calls.append(len(q_))
        return oracle_np.synthetic_kinematic_regressor(q_, ncols, 11)

    Rrand_b, R_b, R_e, names_base, names_e = calculate_base_kinematics_regressor(q, model, None, param,
                                                                                 kinematics_model=kin)
    assert names_base == ref["paramsrand_base"] and names_e == ref["paramsrand_e"]
    assert param["param_name"] == ref["param_name"]
    for got, key in ((Rrand_b, "Rrand_b"), (R_b, "R_b"), (R_e, "R_e")):
        shape, total, abstotal = ref[key]
        assert list(got.shape) == shape
        assert abs(got.sum() - total) <= 1e-12 * abstotal and abs(np.abs(got).sum() - abstotal) <= 1e-12 * abstotal
    # random-configuration regressor from [] for a fixed base, from q for a free-flyer; the given one only if q != 0
    assert calls == ([len(q)] if ref["free_flyer"] else [0]) + ([len(q)] if np.any(q) else [])
    assert "shape of full regressor, reduced regressor, base regressor:" in capsys.readouterr().out
    with pytest.raises(NotImplementedError):
        calculate_base_kinematics_regressor(q, model, None, dict(param))


# ------------------------------------------------------------------------------------------------ flag sweep
@pytest.mark.parametrize("flags", range(8))
def test_regressor_all_flag_combinations(lib, golden, oracle_lib, flags):
    """has_friction / has_actuator_inertia / has_joint_offset in all eight combinations (regressor.py:55-70, :144-169)
    on every config, chain kernel and generic tree kernel, zero pattern included; sign(0) = 0 through a zero velocity."""
    g = golden
    param = dict(g.param, has_friction=bool(flags & 1), has_actuator_inertia=bool(flags & 2),
                 has_joint_offset=bool(flags & 4))
    N = 130
    q = g["q_big"][:N].copy()
    v = g["v_big"][:N].copy()
    a = g["a_big"][:N].copy()
    v[3] = 0.0  # fs column: np.sign(0) = 0
    ref = _oracle_W(g, oracle_lib, q, v, a, param=param)
    for generic in ((False, True) if g.name in ("cfg1_tx40", "cfg2_ur10") else (False,)):
        W = _gpu_W(g, q, v, a, param=param, generic=generic)
        assert W.shape == ref.shape
        assert np.abs(W - ref).max() <= 1e-12 * np.abs(ref).max()
        ext = [c for c in range(ref.shape[1] - (3 if g.coupling else 0)) if c % 14 >= 10]  # Ia fv fs off slots
        assert np.array_equal(W[:, ext], ref[:, ext])  # copies of v, a, sign(v), 1 and zeros: exact


def test_bulk_host_device_copies_roundtrip(lib):
    """figh_memcpy_h2d / figh_memcpy_d2h above 24 MB go through the staged path (32 MB page-locked chunks, eight copy threads):
    ragged sizes around the chunk and page boundaries come back bit-identical, into plain, huge-page-backed (device.host_empty)
    and page-locked destinations; GpuMatrix.numpy() of a padded matrix returns the reference's dense array."""
    from figaroh_plus_amd.device import GpuMatrix, host_empty
    rng = np.random.default_rng(0)
    for n in (3 * (1 << 20) + 5, 4 * (1 << 20), 8 * (1 << 20) + 1, 12345679):  # doubles: 24 MB + 40 B ... 98.8 MB
        src = rng.standard_normal(n)
        d = lib.DeviceArray.from_host(src)
        assert np.array_equal(d.to_host(), src)
        out = host_empty(n)
        lib.check(lib.load().figh_memcpy_d2h(out.ctypes.data, d.ptr, out.nbytes))
        assert np.array_equal(out, src)
        pin = lib.PinnedArray(n)
        lib.check(lib.load().figh_memcpy_d2h(pin.array.ctypes.data, d.ptr, 8 * n))
        assert np.array_equal(pin.array[:n], src)
        d2 = lib.DeviceArray((n,), np.float64)
        lib.check(lib.load().figh_memcpy_h2d(d2.ptr, pin.array.ctypes.data, 8 * n))  # page-locked source: plain DMA
        assert np.array_equal(d2.to_host(), src)
        pin.free()
    # many chunks, position-dependent content (a chunk that lands in the wrong place, or a slice copied from a staging buffer
    # the next DMA has already overwritten, changes the sequence), several repetitions: the pipeline of DMA and copy threads
    n = 50_000_001
    for rep in range(3):
        src = np.arange(n, dtype=np.float64) * (rep + 1.0)
        d = lib.DeviceArray.from_host(src)
        out = host_empty(n) if rep % 2 == 0 else np.empty(n)
        lib.check(lib.load().figh_memcpy_d2h(out.ctypes.data, d.ptr, out.nbytes))
        assert np.array_equal(out, src)
        d.free()
    big = host_empty((9_000_000, 1))
    assert big.flags.writeable and big.flags.c_contiguous and big.ctypes.data % (2 << 20) == 0 and big.base is not None
    A = rng.standard_normal((600_011, 14))
    G = GpuMatrix.from_host(A)
    assert np.array_equal(G.numpy(), A)
    Gp = GpuMatrix.empty(600_011, 14, ld=16)
    lib.check(lib.load().figh_memset(Gp.buf.ptr, 0, Gp.buf.nbytes))
    lib.gather_cols(G.buf, G.rows, G.ld, lib.DeviceArray.from_host(np.arange(14, dtype=np.int32)), 14, Gp.buf, 16)
    assert np.array_equal(Gp.numpy(), A)


# 24 MB + 4, 32 MB + 32772, 32 MB + 32769: the last chunk's floor(n / 8) is a multiple of 4096 and 8 does not divide n -- the
# sizes at which the copy threads' shares (csrc/figh_bulk_copy.h: bulk_slice) once left the last n mod 8 bytes to nobody;
# 32 MB + 32768 is the control on the 8-byte grid
@pytest.mark.parametrize("nbytes", (25_165_828, 33_587_204, 33_587_201, 33_587_200))
def test_bulk_copies_move_every_byte_off_the_8_byte_grid(lib, nbytes):
    """The staged path of figh_memcpy_h2d / figh_memcpy_d2h with byte counts that are no multiple of 8 (uint8; int32 where 4
    divides the count), each direction alone: the other direction is the plain DMA of a page-locked buffer, so a byte that
    one direction drops cannot be put back by the other.  Every destination starts as a sentinel the source never holds and
    has guard bytes behind it, which keep it."""
    from figaroh_plus_amd.device import host_empty
    L, S, G = lib.load(), 0xA5, 64
    src = np.random.default_rng(nbytes).integers(0, S, size=nbytes, dtype=np.uint8)
    if nbytes % 4 == 0:
        src = src.view(np.int32)
    want = src.view(np.uint8)
    pin = lib.PinnedArray((nbytes + G + 7) // 8)
    pinned = pin.array.view(np.uint8)[:nbytes + G]
    d = lib.DeviceArray((nbytes + G,), np.uint8)
    # host -> device alone: staged upload from pageable memory, plain DMA back into the page-locked buffer
    lib.check(L.figh_memset(d.ptr, S, nbytes + G))
    lib.check(L.figh_memcpy_h2d(d.ptr, src.ctypes.data, nbytes))
    pinned[:] = 0
    lib.check(L.figh_memcpy_d2h(pinned.ctypes.data, d.ptr, nbytes + G))
    assert np.array_equal(pinned[:nbytes], want), "h2d: bytes from %d on" % np.flatnonzero(pinned[:nbytes] != want)[0]
    assert np.all(pinned[nbytes:] == S)
    # device -> host alone: plain DMA from the page-locked source, staged download into sentinel-filled pageable memory
    lib.check(L.figh_memset(d.ptr, S, nbytes + G))
    pinned[:nbytes] = want
    lib.check(L.figh_memcpy_h2d(d.ptr, pinned.ctypes.data, nbytes))
    huge = host_empty(8 << 20)  # 64 MB: the huge-page-backed mapping
    assert huge.base is not None
    for out in (np.empty(nbytes + G, dtype=np.uint8), huge.view(np.uint8)[:nbytes + G]):
        out[:] = S
        lib.check(L.figh_memcpy_d2h(out.ctypes.data, d.ptr, nbytes))
        assert np.array_equal(out[:nbytes], want), "d2h: bytes from %d on" % np.flatnonzero(out[:nbytes] != want)[0]
        assert np.all(out[nbytes:] == S)
    d.free()
    pin.free()


def test_device_array_int32_roundtrip_of_24_mb_plus_one_entry(lib):
    """An int32 index list of 6 291 457 entries is 24 MB + 4 bytes: DeviceArray.from_host(...).to_host() returns all of it,
    the last entry included (the one the staged copy dropped in either direction; the destination starts as zeros)."""
    n = 6_291_457
    idx = np.arange(1, n + 1, dtype=np.int32)
    d = lib.DeviceArray.from_host(idx)
    back = d.to_host(out=np.zeros(n, dtype=np.int32))
    assert back[-1] == n
    assert np.array_equal(back, idx)
    d.free()


# ------------------------------------------------------------------------------------------------ two ranks, one GPU
@pytest.mark.timeout(600)
def test_two_process_pipeline_on_one_device(lib, golden_ur10, tmp_path):
    """The N > 1 path of the HIP pipeline on the one GPU a test box has: two FRESH processes (subprocess: nothing that
    has touched the GPU is re-executed), each running IdentificationPipeline on half of the samples with the exchange
    that dist.exchange_from_env negotiates.  Both ranks name the same device, so the collective preflight must rule RCCL
    out on every rank (no rank may be left in ncclCommInitRank) and fall back to the host-staged exchange; column norms
    are all-reduced, the per-rank triangles all-gathered and merged on the device.  Every rank must reproduce the
    reference's idx_e / idx_base / expressions and phi."""
    import json
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    g = golden_ur10
    port = _free_port_pair()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_gpu_worker.py"),
                                       str(tmp_path / ("rank%d.json" % rank))], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=500)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    res = [json.load(open(tmp_path / ("rank%d.json" % r))) for r in range(2)]
    for r in res:
        assert "host-staged" in r["collective"] and "share a device" in r["collective"], r["collective"]
        assert r["idx_e"] == list(g["idx_e"])
        assert r["idx_base"] == list(g["idx_base"])
        assert r["params_base"] == g.meta["params_base"]
        assert r["rows"] == 6 * len(g["q_big"])
        phi = np.array(r["phi_ls"])
        assert np.abs(phi - g["phi_pinv"]).max() <= 1e-6 * np.abs(g["phi_pinv"]).max()
        assert np.abs(np.array(r["col_norm"]) - g["colsq_big"]).max() <= 1e-12 * g["colsq_big"].max()
    assert res[0]["phi_ls"] == res[1]["phi_ls"]  # every rank reduces the same stack: bit-identical results


def _two_device_ranks(tmp_path, models, same_device=False):
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    port = _free_port_pair()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0" if same_device else str(rank),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_rccl_worker.py"),
                                       str(tmp_path / ("rank%d.json" % rank))] + list(models), env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=800)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    return [json.load(open(tmp_path / ("rank%d.json" % r))) for r in range(2)]


def _check_two_rank_results(res, want_rccl):
    from conftest import Golden
    n, nc = 84, 7
    want_sum = sum(np.arange(n, dtype=np.float64) * (r + 1) + 0.25 * r for r in range(2))
    want_stack = np.concatenate([np.triu(np.arange(nc * nc, dtype=np.float64).reshape(nc, nc) + 100.0 * r).reshape(-1)
                                 for r in range(2)])
    A = [np.random.default_rng(40 + r).standard_normal((30 + r, 5)) for r in range(2)]
    for r in res:
        if want_rccl:
            assert r["collective"] == "rccl" and r["exchange_class"] == "RcclExchange", r["collective"]
        else:
            assert "host-staged" in r["collective"] and "share a device" in r["collective"], r["collective"]
        assert np.array_equal(r["sum_columns_device"], want_sum) and np.array_equal(r["sum_columns"], want_sum)
        assert r["stack_count"] == 2 and np.array_equal(r["stack"], want_stack)
        G = sum(a.T @ a for a in A)
        assert np.abs(np.array(r["normal_terms"]["G"]) - G).max() <= 1e-13 * np.abs(G).max()
        assert r["normal_terms"]["rows"] == 61.0
    for cfg in res[0]["models"]:
        g = Golden(cfg)
        a_, b_ = res[0]["models"][cfg], res[1]["models"][cfg]
        assert a_["phi_ls"] == b_["phi_ls"] and a_["absdiagR"] == b_["absdiagR"]  # both ranks reduce the same stack
        for r in (a_, b_):
            assert r["idx_e"] == list(g["idx_e"]) and r["idx_base"] == list(g["idx_base"])
            assert r["params_base"] == g.meta["params_base"]
            ref = g["phi_from_std"]
            assert np.abs(np.array(r["phi_ls"]) - ref).max() <= 1e-6 * np.abs(ref).max()
        if cfg == "cfg2_ur10":
            assert a_["rows"] == 6 * (20000 + 36) and a_["fused_passes"] >= 1  # (equal shards: rows = this rank's x ranks)


@pytest.mark.timeout(900)
def test_two_rank_worker_host_staged_on_one_device(lib, tmp_path):
    """The worker of the two-device RCCL test below with both ranks on device 0: the exchange negotiates itself down to the
    host-staged one, everything else -- primitives, the sharded UR10 (fused) and TALOS (wrench split) passes against the
    golden results -- is the same code, so the two-device test does not meet the worker for the first time on a multi-GPU box."""
    _check_two_rank_results(_two_device_ranks(tmp_path, ["cfg2_ur10", "cfg4_talos"], same_device=True), want_rccl=False)


@pytest.mark.timeout(900)
def test_rccl_two_devices_primitives_and_pipeline(lib, tmp_path):
    """RCCL with N > 1 on real hardware (skipped on a one-GPU box): two fresh processes, rank r on device
    r, exchange negotiated by dist.exchange_from_env over the socket control plane -- it must be RcclExchange.  Primitives on
    device buffers: all-reduce of column norms (in place and returned), all-gather of the per-rank triangles in rank order,
    the packed normal-terms all-reduce with unequal shards.  Then one sharded IdentificationPipeline pass per model -- UR10
    (fused launch, narrow merge tree) and TALOS (wrench split, wide pair merges) -- against the golden idx_e / idx_base /
    expressions / phi; both ranks reduce the same stack and must agree bit for bit."""
    if lib.device_count() < 2:
        pytest.skip("needs two GPUs (the driver's GPU test box has one); the same path is covered host-staged by "
                    "test_two_process_pipeline_on_one_device and on CPU by tests/test_dist_cpu.py")
    _check_two_rank_results(_two_device_ranks(tmp_path, ["cfg2_ur10", "cfg4_talos"]), want_rccl=True)


def test_sharded_pass_on_random_models_with_a_replay_exchange(lib):
    """The collective code paths of the pipeline (all-reduced norms, non-local rank decision, stacked triangles through
    figh_tsqr_merge_base) on random models in ONE process: tools/fuzz_sharded.py splits the samples into two or three unequal
    shards, runs one pipeline per shard under an exchange of world size > 1 that replays the other shards' contributions, and
    compares with the single-rank pass on all samples -- serial chains (fused launch), fixed-base trees (per-row-block TSQR,
    both layouts), floating-base trees (force / torque split).  900 seeds in round 6; twelve here."""
    import subprocess
    import sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_sharded.py"), "0", "12"], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=600).stdout.decode()
    assert "12 sharded random models (seeds 0 .. 11), 0 failures" in out, out[-3000:]


def test_bench_two_ranks_share_the_device(lib):
    """bench.py as the driver launches it for N > 1 (torch.distributed.run, one process per rank), on the one GPU a test
    box has: both ranks drive device 0, so the exchange must be negotiated down to the host-staged one on every rank
    (the device key is the device actually bound, LOCAL_RANK modulo the device count -- a launch with distinct
    LOCAL_RANKs on one device used to walk into ncclCommInitRank and fail), the line must be the weak-scaling one with
    n_gpus = 2 and the step must reproduce the reference's structural result; then the strong-scaling TALOS mode."""
    import json
    import socket
    import subprocess
    import sys
    from conftest import ROOT

    def run(extra):
        port = _free_port_pair()
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        for k in [k for k in env if k.startswith("FIGH_")]:
            del env[k]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
               "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--strong-config", ""] + extra
        out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900).stdout.decode()
        lines = [l for l in out.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out[-3000:]
        return json.loads(lines[0])

    d = run(["--steps", "3", "--warmup", "1", "--samples", "200000"])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["samples_total"] == 400000
    assert d["config"]["ranks"] == 2 and d["config"]["host_wait"] == "block"
    assert "share a device" in d["config"]["collective"] and d["config"]["result_matches_reference"] is True
    assert abs(d["value"] - 400000 * 3 / d["config"]["max_rank_seconds"]) <= 1e-6 * d["value"]
    d = run(["--config", "cfg4", "--steps", "1", "--warmup", "1", "--samples", "200000"])
    assert d["scaling"] == "strong" and d["config"]["samples_this_rank"] == 100000 and d["config"]["samples_total"] == 200000
    assert d["config"]["result_matches_reference"] is True


def test_bench_spawns_its_own_ranks(lib):
    """`python bench.py --gpus 2` with NO launcher (WORLD_SIZE unset): bench.py starts two fresh rank processes itself
    (bench.spawn_ranks: the parent never touches the GPU), the ranks meet over the socket control plane, rank 0 prints ONE
    line with ranks = 2; on the one-GPU box both ranks share the device (host-staged exchange).  The line carries the
    strong-scaling measurement of TALOS beside the weak-scaling headline."""
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if not k.startswith("FIGH_") and k not in (
        "RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--samples", "200000",
           "--strong-samples", "200000", "--strong-steps", "2"]
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = proc.stdout.decode()
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert proc.returncode == 0 and len(lines) == 1, out[-3000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["ranks"] == 2 and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["config"]["samples_total"] == 400000 and d["config"]["result_matches_reference"] is True
    if lib.device_count() < 2:
        assert "share a device" in d["config"]["collective"]
    else:
        assert d["config"]["collective"] == "rccl"
    ss = d["strong_scaling"]
    assert ss["scaling"] == "strong" and ss["n_gpus"] == 2 and ss["config"]["samples_total"] == 200000
    assert ss["config"]["samples_this_rank"] == 100000 and ss["config"]["result_matches_reference"] is True
    # a rank that fails takes the run down with a non-zero exit code instead of leaving its peer at a barrier
    bad = subprocess.run(cmd + ["--config", "cfg9"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert bad.returncode != 0


def test_bench_two_ranks_socket_rendezvous(lib):
    """bench.py with --rendezvous socket, launched WITHOUT torch.distributed.run: two plain processes with RANK / WORLD_SIZE /
    MASTER_* in their environment (any launcher can do that), control plane = figaroh_plus_amd.dist.SocketGroup.  Both ranks
    share the box's one GPU, so the exchange is negotiated down to the host-staged one; the line is the weak-scaling one."""
    import json
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    port = _free_port_pair()
    procs = []
    for rank in range(2):
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2",
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        for k in [k for k in env if k.startswith("FIGH_")]:
            del env[k]
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--strong-config", "", "--steps", "3",
                                       "--warmup", "2", "--samples", "200000", "--rendezvous", "socket"], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=900)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs[0][-2000:] + outs[1][-2000:]
    lines = [l for l in outs[0].splitlines() if l.startswith("{")]
    assert len(lines) == 1 and not [l for l in outs[1].splitlines() if l.startswith("{")]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["samples_total"] == 400000
    assert "socket control plane" in d["config"]["collective"] and "share a device" in d["config"]["collective"]
    assert d["config"]["result_matches_reference"] is True


def test_tsqr_randomised_stress(lib):
    """tools/tsqr_stress.py: 60 random cases over the blocked-kernel range (column counts on and off the geometry
    boundaries, ragged and short row counts, column gathers, tau, row-block weights, zero leading blocks, exactly
    dependent columns whose pivots must come out at rounding level) -- run as a child process with a fixed seed."""
    import subprocess
    import sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "tsqr_stress.py"), "60", "20250410"],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode == 0 and b"all 60 cases ok" in out.stdout, out.stdout.decode()[-2000:]


# ------------------------------------------------------------------------------------------------ round 3: no host round trip
def _rows_to_blocks(rows_k, n, tol):
    d = np.abs(rows_k[-1])
    rows_k = rows_k[:-1]
    base = np.flatnonzero(d[:n] > tol)
    rest = np.flatnonzero(~(d[:n] > tol))
    Rb = rows_k[base]
    return base, rest, np.triu(Rb[:, base]), Rb[:, rest], d


@pytest.mark.parametrize("stride", [14, 16])
def test_select_columns_on_device(lib, stride):
    """get_index_eliminate (regressor.py:258-279) on the device: mask, compacted list in W's numbering, NaN kept."""
    rng = np.random.default_rng(3)
    for ncols in (1, 14, 84, 87 if stride == 14 else 96, 560):
        cs = rng.uniform(0.0, 2e-6, ncols)
        cs[rng.integers(0, ncols, 3)] = 0.0
        if ncols > 20:
            cs[7] = np.nan
            cs[11] = 1e-6  # not < tol: kept
        d_cs = lib.DeviceArray.from_host(cs)
        d_sel = lib.DeviceArray((2 + 2 * ncols,), np.int32)
        lib.select_columns(d_cs, ncols, 1e-6, stride, d_sel)
        sel = d_sel.to_host()
        kept = np.flatnonzero(~(cs < 1e-6))
        assert sel[0] == len(kept) and sel[1] == ncols
        assert np.array_equal(sel[2:2 + len(kept)], (kept // 14) * stride + kept % 14)
        assert not sel[2 + len(kept):2 + ncols].any()
        assert np.array_equal(sel[2 + ncols:] != 0, ~(cs < 1e-6))


@pytest.mark.parametrize("nc,count", [(1, 5), (17, 40), (50, 2), (50, 16), (50, 300), (50, 2039), (64, 700), (65, 9), (80, 130),
                                      (49, 4500), (81, 2), (120, 7), (191, 33), (241, 5), (331, 16), (336, 3), (400, 2),
                                      (511, 3)])
def test_merge_tree_against_lapack(lib, nc, count):
    """figh_tsqr_merge: every level in one launch (figh_tsqr_tree.hip) -- one, two and three levels, both tile
    geometries, and the stack that is too tall for one resident grid (4500 triangles: per-level launches); nc > 80: the
    pair-merge levels of the blocked kernel (a workgroup starts from one triangle and absorbs the next; odd counts pass
    the last triangle through), every geometry."""
    rng = np.random.default_rng(nc * 1000 + count)
    stack = np.triu(rng.standard_normal((count, nc, nc)))
    stack[:, :, nc // 2] *= 1e-3
    d_stack = lib.DeviceArray.from_host(stack.reshape(-1))
    d_R = lib.DeviceArray((nc * nc,))
    lib.tsqr_merge(d_stack, count, nc, d_R)
    R = d_R.to_host().reshape(nc, nc)
    assert np.array_equal(R, np.triu(R))
    ref = np.linalg.qr(stack.reshape(-1, nc), mode="r")
    assert np.abs(np.abs(R) - np.abs(ref)).max() <= 1e-12 * np.abs(ref).max()
    # ... and column by column: the 1e-3-scaled column is held to its own size, not to 1e-9 of it
    cn = np.linalg.norm(stack.reshape(-1, nc), axis=0)
    assert (np.abs(np.abs(R) - np.abs(ref)).max(axis=0) <= 1e-12 * cn).all()
    # bit-reproducible
    lib.tsqr_merge(d_stack, count, nc, d_R)
    assert np.array_equal(d_R.to_host().reshape(nc, nc), R)


@pytest.mark.parametrize("nc,count,with_tau", [(50, 1, True), (50, 8, True), (37, 200, False), (70, 33, True), (50, 2039, True),
                                               (120, 3, True), (200, 1, False)])
def test_merge_base_rank_revealing_level(lib, nc, count, with_tau):
    """figh_tsqr_merge_base: the rows of qr([W1 W2 tau]) in the original column order + the pivots of the plain
    factorisation, against NumPy on the same stack (qrdecomposition.py:205-244)."""
    rng = np.random.default_rng(nc + count)
    n = nc - (1 if with_tau else 0)
    # a stack whose columns have exact dependencies: every third column is a combination of earlier ones
    rows = max(4 * nc, count * nc)
    A = rng.standard_normal((rows, nc))
    dep = [k for k in range(2, n) if k % 3 == 2]
    for k in dep:
        A[:, k] = A[:, :k] @ rng.standard_normal(k) * 0.3
    parts = np.array_split(A, count)
    stack = np.stack([np.linalg.qr(p, mode="r") if p.shape[0] >= nc else
                      np.vstack([np.linalg.qr(p, mode="r"), np.zeros((nc - p.shape[0], nc))]) for p in parts])
    d_stack = lib.DeviceArray.from_host(stack.reshape(-1))
    d_out = lib.DeviceArray(((nc + 1) * nc,))
    tol = 1e-8
    lib.tsqr_merge_base(d_stack, count, nc, n, tol, d_out)
    rows_k = d_out.to_host().reshape(nc + 1, nc)
    base, rest, R1, R2, d = _rows_to_blocks(rows_k, n, tol)
    Rp = np.linalg.qr(A, mode="r")
    assert base.tolist() == [k for k in range(n) if k not in dep]
    assert base.tolist() == np.flatnonzero(np.abs(np.diag(Rp))[:n] > tol).tolist()
    # diagonal of the plain factorisation.  Up to the first dependent column it is LAPACK's; behind it every
    # implementation's reflector of a dependent column points along its own rounding noise and takes a different (small)
    # part of the later columns with it, so only |R_kk| <= dist(column k, span of the base columns before it) = |R1_ii|
    # is implementation independent there.  Dependent columns sit at roundoff level.
    dp = np.abs(np.diag(Rp))
    first_dep = dep[0] if dep else n
    assert np.abs(d[:first_dep] - dp[:first_dep]).max() <= 1e-11 * dp.max()
    assert (d[base] <= np.abs(np.diag(R1)) * (1 + 1e-11)).all() and d[base].min() > 1e-3
    assert d[rest].max(initial=0.0) <= 1e-10 * dp.max()
    rows_k = rows_k[:nc]
    # regrouped factorisation
    perm = base.tolist() + rest.tolist() + ([n] if with_tau else [])
    Rr = np.linalg.qr(A[:, perm], mode="r")
    r = len(base)
    assert np.abs(np.abs(R1) - np.abs(Rr[:r, :r])).max() <= 1e-11 * np.abs(Rr).max()
    beta = np.linalg.solve(R1, R2)
    beta_ref = np.linalg.solve(Rr[:r, :r], Rr[:r, r:n])
    assert np.abs(beta - beta_ref).max() <= 1e-9 * max(1.0, np.abs(beta_ref).max())
    assert not rows_k[rest].any()  # rows of dependent columns are empty
    if with_tau:
        phi = np.linalg.solve(R1, rows_k[base][:, n])
        phi_ref = np.linalg.lstsq(A[:, base], A[:, n], rcond=None)[0]
        assert np.abs(phi - phi_ref).max() <= 1e-9 * max(1.0, np.abs(phi_ref).max())
        res = np.linalg.norm(A[:, n] - A[:, base] @ phi_ref)
        assert abs(abs(rows_k[n, n]) - res) <= 1e-9 * max(1.0, res)


def test_tsqr_selected_matches_host_flow(lib, golden):
    """figh_tsqr_selected: elimination + TSQR + rank-revealing merge without a host round trip == the reference's
    sequence get_index_eliminate -> build_regressor_reduced -> get_baseParams on the same W (all five configs; chains in
    the reference layout with the structure hint, trees in the link-padded layout)."""
    from figaroh_plus_amd.tools.regressor import build_regressor_device, regressor_flags
    g = golden
    robot = g.robot()
    q, v, a = g["q_big"], g["v_big"], g["a_big"]
    N = len(q)
    dq, dv, da = (lib.DeviceArray.from_host(np.ascontiguousarray(x).reshape(-1)) for x in (q, v, a))
    W, colsq = build_regressor_device(robot, dq, dv, da, N, g.param, coupling=g.coupling, colsq=True)
    ncols = W.cols
    mode, _, _ = regressor_flags(g.param, g.coupling)
    m = robot.model
    nblocks = m.nv if (mode == lib.MODE_JOINT_TORQUE and m.nv == m.njoints - 1 and N >= 64) else 0
    d_tau = lib.DeviceArray.from_host(g["tau"])
    d_sel = lib.DeviceArray((2 + 2 * ncols,), np.int32)
    # selection only (count unknown), then a stale count, then the right one
    lib.tsqr_selected(W.buf, W.rows, W.ld, colsq, ncols, 1e-6, 14, nblocks, -1, d_tau, 1e-8, d_sel, None)
    sel = d_sel.to_host()
    kept = [i for i in range(ncols) if i not in set(g["idx_e"].tolist())]
    n = len(kept)
    assert sel[0] == n and sel[2:2 + n].tolist() == kept
    d_rows = lib.DeviceArray(((n + 2) * (n + 1),))
    lib.tsqr_selected(W.buf, W.rows, W.ld, colsq, ncols, 1e-6, 14, nblocks, n - 1, d_tau, 1e-8, d_sel, d_rows)
    assert d_sel.to_host()[0] == n  # the device reports its own count whatever the caller expected
    lib.tsqr_selected(W.buf, W.rows, W.ld, colsq, ncols, 1e-6, 14, nblocks, n, d_tau, 1e-8, d_sel, d_rows)
    rows_k = d_rows.to_host().reshape(n + 2, n + 1)
    base, rest, R1, R2, d = _rows_to_blocks(rows_k, n, 1e-8)
    assert base.tolist() == list(g["idx_base"])
    beta = np.around(np.linalg.solve(R1, R2), 6)
    from figaroh_plus_amd.tools.qrdecomposition import _expressions
    params_r = g.meta["params_r"]
    assert _expressions([params_r[i] for i in base], [params_r[i] for i in rest], beta) == g.meta["params_base"]
    phi = np.linalg.solve(R1, rows_k[base][:, n])
    assert np.abs(phi - g["phi_pinv"]).max() <= 1e-6 * np.abs(g["phi_pinv"]).max()
    # plain triangle (tol < 0) == figh_tsqr on the same columns
    d_R = lib.DeviceArray(((n + 1) * (n + 1),))
    lib.tsqr_selected(W.buf, W.rows, W.ld, colsq, ncols, 1e-6, 14, nblocks, n, d_tau, -1.0, d_sel, d_R)
    R = d_R.to_host().reshape(n + 1, n + 1)
    d_idx = lib.DeviceArray.from_host(np.asarray(kept, dtype=np.int32))
    d_R2 = lib.DeviceArray(((n + 1) * (n + 1),))
    lib.tsqr(W.buf, W.rows, W.ld, d_idx, n, d_tau, None, d_R2)
    R2_ = d_R2.to_host().reshape(n + 1, n + 1)
    assert np.abs(np.abs(R) - np.abs(R2_)).max() <= 1e-11 * np.abs(R2_).max()
    assert np.abs(np.abs(np.diag(R)) - d).max() <= 1e-11 * d.max()


def test_pipeline_recovers_when_the_kept_set_changes(lib, golden_ur10):
    """The pass is launched with the previous pass's column count; data with another elimination pattern must be
    detected from the device's own count and solved again (no stale shape, no stale list)."""
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from figaroh_plus_amd.tools.regressor import build_regressor_basic, get_index_eliminate
    from figaroh_plus_amd.tools.qrdecomposition import get_baseIndex
    g = golden_ur10
    pipe = IdentificationPipeline(g.robot(), g.param, params_std=g.params_std(), coupling=g.coupling)
    q, v, a = g["q_big"].copy(), g["v_big"].copy(), g["a_big"].copy()
    pipe.set_samples(q, v, a, g["tau"])
    out = pipe.run()
    assert out["idx_e"] == list(g["idx_e"])
    # same pipeline object, same HBM buffers: overwrite the samples in place with a motion of the last three joints only
    q2, v2, a2 = q.copy(), v.copy(), a.copy()
    q2[:, :3] = 0.0
    v2[:, :3] = 0.0
    a2[:, :3] = 0.0
    for d_arr, h in ((pipe.d_q, q2), (pipe.d_v, v2), (pipe.d_a, a2)):
        h = np.ascontiguousarray(h)
        lib.check(lib.load().figh_memcpy_h2d(d_arr.ptr, h.ctypes.data, h.nbytes))
    out2 = pipe.run()
    W2 = build_regressor_basic(g.robot(), q2, v2, a2, g.param)
    idx_e2, params_r2 = get_index_eliminate(W2, g.params_std(), 1e-6)
    assert out2["idx_e"] == idx_e2 and out2["params_r"] == params_r2
    assert len(idx_e2) != len(g["idx_e"])
    keep = [i for i in range(W2.shape[1]) if i not in set(idx_e2)]
    assert out2["idx_base"] == list(get_baseIndex(np.ascontiguousarray(W2[:, keep]), params_r2))
    out3 = pipe.run()
    assert out3["idx_base"] == out2["idx_base"] and np.array_equal(out3["beta"], out2["beta"])


@pytest.mark.parametrize("freeflyer", [False, True])
def test_handwritten_robot_against_first_principles(lib, tmp_path, freeflyer):
    """The HIP regressor (tape kernel: branches, continuous / revolute / prismatic joints, merged fixed link, free-flyer
    wrench rows) behind build_regressor_basic + Robot.get_standard_parameters against tests/indep_dynamics.py -- subtree
    momenta differentiated numerically, no spatial algebra -- on 45 instances of a hand-written robot whose inertial data
    span every parameter: W(q, v, a) . phi_std == tau for all of them pins every column of the device's W on physics,
    with the product's own URDF loader in the loop."""
    import indep_dynamics as idyn
    from figaroh_plus_amd.tools.regressor import build_regressor_basic
    from figaroh_plus_amd.tools.robot import Robot
    param = {"is_joint_torques": not freeflyer, "is_external_wrench": freeflyer, "force_torque": ["All"],
             "has_friction": False, "has_actuator_inertia": False, "has_joint_offset": False}
    rng = np.random.default_rng(21 + int(freeflyer))
    N = 6
    states = [idyn.sample_state(rng, freeflyer) for _ in range(N)]
    q, v, a = (np.array([s[i] for s in states]) for i in range(3))
    W0, PHI, TAU = None, [], []
    for k in range(45):
        ine = idyn.random_inertials(rng)
        path = os.path.join(str(tmp_path), "b3_%d.urdf" % k)
        with open(path, "w") as f:
            f.write(idyn.urdf_text(ine))
        robot = Robot(path, isFext=freeflyer)
        if W0 is None:
            W0 = build_regressor_basic(robot, q, v, a, param)  # kinematics only: the same for every instance
        PHI.append(np.array(list(robot.get_standard_parameters(param).values()), dtype=float))
        tau = np.array([idyn.generalised_forces(ine, *s, freeflyer) for s in states])  # N x nv
        TAU.append((tau[:, :6] if freeflyer else tau).T.reshape(-1))                    # rows c * N + i, as W
    PHI, TAU = np.array(PHI), np.array(TAU)
    inertial = [c for c in range(W0.shape[1]) if c % 14 < 10]
    assert np.linalg.matrix_rank(PHI[:, inertial]) == len(inertial)
    assert not W0[:, [c for c in range(W0.shape[1]) if c % 14 >= 10]].any()
    err = np.abs(PHI @ W0.T - TAU).max()
    assert err <= 2e-7 * np.abs(TAU).max(), err
    Wrec = np.linalg.lstsq(PHI[:, inertial], TAU, rcond=None)[0].T
    assert np.abs(Wrec - W0[:, inertial]).max() <= 1e-5 * np.abs(W0).max()


@pytest.mark.parametrize("n", [50, 70, 81, 96, 191, 241, 305, 331, 400, 511])
def test_tsqr_ragged_rows_inside_a_nan_filled_buffer(lib, n):
    """the blocked kernel zero-fills the rows of a ragged last tile through the range check of its buffer
    descriptor (and the register-tile kernel clamps and masks them).  W is therefore placed as the first `rows` rows of a
    larger allocation whose remainder -- and tau's -- is NaN: nothing behind the matrix may reach the result, for every
    tile geometry and with a padded leading dimension."""
    from figaroh_plus_amd.pipeline import _View
    rng = np.random.default_rng(n)
    for rows, ld in ((1000 + 37, n), (20011, n + 5)):
        A = rng.standard_normal((rows, n)) * rng.uniform(0.5, 20.0, n)
        t = rng.standard_normal(rows)
        extra = 200
        buf = np.full((rows + extra, ld), np.nan)
        buf[:rows, :n] = A
        tb = np.full(rows + extra, np.nan)
        tb[:rows] = t
        d_buf, d_tau = lib.DeviceArray.from_host(buf.reshape(-1)), lib.DeviceArray.from_host(tb)
        d_R = lib.DeviceArray(((n + 1) * (n + 1),))
        d_idx = lib.DeviceArray.from_host(np.arange(n, dtype=np.int32))
        lib.tsqr(_View(d_buf, 0), rows, ld, d_idx, n, d_tau, None, d_R)
        R = d_R.to_host().reshape(n + 1, n + 1)
        assert np.isfinite(R).all()
        At = np.c_[A, t]
        G = At.T @ At
        assert np.abs(R.T @ R - G).max() <= 1e-12 * np.abs(G).max()


def test_pipeline_through_rccl_exchange_of_one_rank(lib, golden_ur10):
    """The device-buffer exchange path of the pipeline (all-reduce of the column norms in HBM, device-side selection,
    plain local triangle, all-gather into the stack, rank decision on the merged stack) executed through RcclExchange
    itself -- a communicator of one rank on the one GPU of the test box -- and compared with the single-process pass."""
    from figaroh_plus_amd.dist import RcclExchange, rccl_unique_id
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    g = golden_ur10
    ref = IdentificationPipeline(g.robot(), g.param, params_std=g.params_std(), coupling=g.coupling)
    ref.set_samples(g["q_big"], g["v_big"], g["a_big"], g["tau"])
    out0 = ref.run()
    ex = RcclExchange(1, 0, rccl_unique_id())
    try:
        pipe = IdentificationPipeline(g.robot(), g.param, params_std=g.params_std(), coupling=g.coupling, exchange=ex)
        pipe.set_samples(g["q_big"], g["v_big"], g["a_big"], g["tau"])
        for _ in range(2):
            out = pipe.run()
            assert out["idx_e"] == out0["idx_e"] and out["idx_base"] == out0["idx_base"] == list(g["idx_base"])
            assert out["params_base"] == g.meta["params_base"]
            assert np.array_equal(out["col_norm"], out0["col_norm"])
            assert np.abs(out["phi_ls"] - out0["phi_ls"]).max() <= 1e-9 * np.abs(out0["phi_ls"]).max()
            assert abs(out["residual_norm"] - out0["residual_norm"]) <= 1e-9 * out0["residual_norm"]
    finally:
        ex.close()


@pytest.mark.parametrize("N,width", [(1, 5), (63, 39), (64, 38), (65, 7), (400, 46), (1000, 1)])
def test_repack_samples_layout(lib, N, width):
    """figh_repack_samples: [tile of 64 samples][value][lane], the last tile padded with its last sample."""
    rng = np.random.default_rng(N + width)
    x = rng.standard_normal((N, width))
    d = lib.repack_samples(lib.DeviceArray.from_host(x.reshape(-1)), N, width)
    got = d.to_host().reshape(-1, width, 64)
    nt = (N + 63) // 64
    pad = np.concatenate([x, np.repeat(x[-1:], nt * 64 - N, axis=0)]).reshape(nt, 64, width).transpose(0, 2, 1)
    assert np.array_equal(got, pad)


def test_tree_regressor_blocked_inputs_identical(lib, golden):
    """FIGH_FLAG_BLOCKED_INPUTS: the generic-tree kernel on the tile-blocked copies of q, v, a writes the same W and the
    same column norms, bit for bit, as on the reference's sample-major arrays (all models through the tape kernel; chains
    with the generic-kernel flag; ragged last tile)."""
    from figaroh_plus_amd.tools.regressor import regressor_flags
    g = golden
    robot = g.robot()
    m = robot.model
    q, v, a = g["q_big"], g["v_big"], g["a_big"]
    N = len(q)
    mode, flags, ft = regressor_flags(dict(g.param, force_generic_kernel=True), g.coupling)
    dm = robot.device_model()
    rps, ncols = dm.shape(mode, flags)
    dq, dv, da = (lib.DeviceArray.from_host(np.ascontiguousarray(x).reshape(-1)) for x in (q, v, a))
    bq, bv, ba = lib.repack_samples(dq, N, m.nq), lib.repack_samples(dv, N, m.nv), lib.repack_samples(da, N, m.nv)
    outs = []
    for (xq, xv, xa), fl in (((dq, dv, da), flags), ((bq, bv, ba), flags | lib.FLAG_BLOCKED_INPUTS)):
        W = lib.DeviceArray((rps * N * ncols,))
        cs = lib.DeviceArray((ncols,))
        lib.regressor_build(dm, mode, fl, ft, N, xq, xv, xa, W, ncols, cs)
        outs.append((W.to_host(), cs.to_host()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    if not g.coupling and not (dm.is_chain() and mode == lib.MODE_JOINT_TORQUE):
        ld = 16 * (m.njoints - 1)
        outs = []
        for (xq, xv, xa), fl in (((dq, dv, da), flags & 7), ((bq, bv, ba), (flags & 7) | lib.FLAG_BLOCKED_INPUTS)):
            W = lib.DeviceArray((rps * N * ld,))
            cs = lib.DeviceArray((ncols,))
            lib.regressor_build_padded(dm, mode, fl, ft, N, xq, xv, xa, W, ld, cs)
            outs.append((W.to_host(), cs.to_host()))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    else:
        with pytest.raises(lib.FighError):  # the chain kernel keeps the original arrays
            lib.regressor_build(dm, mode, (flags & ~lib.FLAG_GENERIC) | lib.FLAG_BLOCKED_INPUTS, ft, N, bq, bv, ba,
                                lib.DeviceArray((rps * N * ncols,)), ncols, None)


# ------------------------------------------------------------------------------------------------ fused K1 + TSQR
def _ur10_problem(g, N, seed, noise=0.05):
    rng = np.random.default_rng(seed)
    q, v, a = (rng.uniform(-6, 6, (N, 6)) for _ in range(3))
    return q, v, a, rng, noise


@pytest.mark.parametrize("N", [4096, 20000, 20037, 131072 + 5])
def test_fused_pass_equals_two_launch_pass(lib, golden_ur10, N):
    """figh_regressor_tsqr_fused (K1 + level-0 TSQR in one launch, tiles factored out of LDS) against the two-launch pass on
    the same samples: W to a few ulp with the identical zero pattern, diag(W^T W) to 1e-13, identical index sets and expressions, R up to rounding (the tiles of a CU go to
    whichever consumer wave is free: the grouping of rows into triangles differs from the two-launch kernel's and from run
    to run), phi to 1e-9."""
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    g = golden_ur10
    q, v, a, rng, noise = _ur10_problem(g, N, 77 + N)
    phi = g.phi_ref()
    outs, Ws, pipes = [], [], []
    for fuse in (False, True):
        pipe = IdentificationPipeline(g.robot(), g.param, params_std=g.params_std(), coupling=g.coupling, fuse=fuse)
        pipe.set_samples(q, v, a)
        pipe.set_tau_from_parameters(phi, noise_std=noise, seed=3)
        pipe.run()
        # poison W: the second pass must re-create every byte
        lib.check(lib.load().figh_memset(pipe.W.buf.ptr, 0xff, pipe.W.rows * pipe.W.ld * 8))
        out = pipe.run()
        assert pipe.fused_passes == (2 if fuse else 0)  # (the first pass is fused as well: kept set from a 4096-sample prefix)
        W = np.empty((pipe.W.rows, pipe.W.ld))
        lib.check(lib.load().figh_memcpy_d2h(W.ctypes.data, pipe.W.buf.ptr, W.nbytes))
        outs.append(out)
        Ws.append(W)
        pipes.append(pipe)
    a_, b_ = outs
    # the same formulas, compiled in another context (the fused producer re-forms the link rotations per row where the
    # two-launch kernel keeps them): products are contracted differently here and there, entries agree to a few ulp
    assert np.abs(Ws[0] - Ws[1]).max() <= 4e-16 * np.abs(Ws[0]).max(), "fused W differs from the two-launch W"
    assert np.array_equal(Ws[0] == 0.0, Ws[1] == 0.0)
    assert np.abs(a_["col_norm"] - b_["col_norm"]).max() <= 1e-13 * a_["col_norm"].max()
    assert a_["idx_e"] == b_["idx_e"] == list(g["idx_e"])
    assert a_["params_r"] == b_["params_r"]
    assert a_["idx_base"] == b_["idx_base"] == list(g["idx_base"])
    assert a_["params_base"] == b_["params_base"] == g.meta["params_base"]
    # |R_kk| is unique up to the first dependent column only (behind it no two Householder orders agree)
    first_dep = min(i for i in range(len(a_["params_r"])) if i not in set(a_["idx_base"]))
    d_a, d_b = a_["absdiagR"][:first_dep], b_["absdiagR"][:first_dep]
    assert np.abs(d_a - d_b).max() <= 1e-11 * d_a.max()
    assert np.abs(a_["phi_ls"] - b_["phi_ls"]).max() <= 1e-9 * np.abs(a_["phi_ls"]).max()
    assert abs(a_["residual_norm"] - b_["residual_norm"]) <= 1e-11 * a_["residual_norm"]
    assert np.array_equal(a_["beta"], b_["beta"])
    # a third pass: fused again, same results up to rounding
    c_ = pipes[1].run()
    assert pipes[1].fused_passes == 3
    assert c_["idx_base"] == b_["idx_base"] and np.abs(c_["phi_ls"] - b_["phi_ls"]).max() <= 1e-10 * np.abs(b_["phi_ls"]).max()


def test_fused_pass_twice_is_reproducible_within_rounding(lib, golden_ur10):
    """The fused launch deals tiles to whichever consumer wave is free, so the grouping of rows into level-0 triangles -- and
    with it the rounding of R -- differs from run to run.  What a caller can rely on: over repeated passes
    on the same samples the index sets are identical and R^T R (which is W_kept^T W_kept whatever the grouping) agrees to
    1e-12 of its scale; checked over five fused passes against the first one."""
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    g = golden_ur10
    q, v, a, rng, noise = _ur10_problem(g, 200000, 911)
    pipe = IdentificationPipeline(g.robot(), g.param, params_std=g.params_std(), coupling=g.coupling)
    pipe.set_samples(q, v, a)
    pipe.set_tau_from_parameters(g.phi_ref(), noise_std=noise, seed=5)
    pipe.run()
    grams, outs = [], []
    for rep in range(5):
        out = pipe.run()
        n = len(out["params_r"])
        kept = pipe._fused_kept[1]
        d_R = lib.DeviceArray(((n + 1) * (n + 1),), np.float64)
        assert lib.regressor_tsqr_fused(pipe.robot.device_model(), pipe._flags()[1], pipe.N, pipe.d_q, pipe.d_v, pipe.d_a,
                                        pipe.W.buf, pipe.W.ld, pipe._d_colsq, kept, n, pipe.d_tau, -1.0, d_R)
        R = np.triu(d_R.to_host().reshape(n + 1, n + 1))
        grams.append(R.T @ R)
        outs.append(out)
    assert pipe.fused_passes == 6
    scale = np.abs(grams[0]).max()
    for G, out in zip(grams[1:], outs[1:]):
        assert np.abs(G - grams[0]).max() <= 1e-12 * scale
        assert out["idx_e"] == outs[0]["idx_e"] and out["idx_base"] == outs[0]["idx_base"]
        assert out["params_base"] == outs[0]["params_base"] and np.array_equal(out["beta"], outs[0]["beta"])
        assert np.abs(out["phi_ls"] - outs[0]["phi_ls"]).max() <= 1e-10 * np.abs(outs[0]["phi_ls"]).max()


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("cfg,sizes", [("cfg3_tiago", (200000, 400000)), ("cfg1_tx40", (50000,))])
def test_null_pivot_rule_never_changes_the_base_set(lib, cfg, sizes):
    """The null-pivot rule (include/figh.h, on by default in the pipeline) against plain Householder on the models whose
    pivots come closest to tol_qr: TIAGo (four + two "dependent" pivots within a factor 1.5 of the tolerance at 4e5 samples,
    tests/golden/cfg3_tiago_large.json) and the TX40 with its coupling columns -- three seeds each, rule on / off: identical
    idx_e and idx_base, phi_b to 1e-6, and every dependent pivot is either far below the tolerance (<= tol_qr / 2: rounding
    residue, whatever the rule folded into it) or a genuine near-tolerance pivot, which the rule must leave alone (equal
    to 1e-3 in both modes).  (Was tools/null_rank_sweep.py, 21 cases by hand: VERDICT r04.)"""
    from conftest import Golden
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from figaroh_plus_amd.tools.qrdecomposition import TOL_QR
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    g = Golden(cfg)
    robot = g.robot()
    layout = "block-compact" if cfg == "cfg3_tiago" else "dense"
    for N in sizes:
        for seed in (1, 2, 3):
            rng = np.random.default_rng(1000 * seed + N // 1000)
            if cfg == "cfg1_tx40":
                q, v, a = rng.uniform(-6, 6, (N, 6)), rng.uniform(-10, 10, (N, 6)), rng.uniform(-30, 30, (N, 6))
            else:
                q, v, a = sample_inputs(robot.model, N, rng, 1.5, 2, 5)
            res = {}
            for on in (False, True):
                pipe = IdentificationPipeline(robot, g.param, params_std=g.params_std(), coupling=g.coupling, w_layout=layout,
                                              null_pivots=on)
                pipe.set_samples(q, v, a)
                pipe.set_tau_from_parameters(g.phi_ref(), noise_std=0.05, seed=seed)
                pipe.run()
                res[on] = pipe.run()
                del pipe
            off, on_ = res[False], res[True]
            assert on_["idx_e"] == off["idx_e"] and on_["idx_base"] == off["idx_base"], (cfg, N, seed)
            # (the regrouping coefficients agree to a few units of their 6-decimal rounding; the expression STRINGS list every
            # term of at least 1e-6, and with 50 000 random TX40 samples both modes carry a few noise terms of exactly that
            # size -- different ones -- so the strings are compared where no coefficient sits at the threshold)
            assert np.abs(on_["beta"] - off["beta"]).max() <= 5e-6
            if not ((np.abs(off["beta"]) > 0) & (np.abs(off["beta"]) < 1e-5)).any():
                assert on_["params_base"] == off["params_base"]
            # (with random samples both base regressors are ill-conditioned -- TIAGo: one base parameter comes out at 4e6 with
            # 0.05 of noise on tau, TX40 with its coupling columns at 1e5 -- and ANY two Householder orders differ by
            # cond(W_b) eps in phi: the fit itself, the residual, is what is compared to 1e-9)
            # (round 6: the bound is the conditioning the run itself reports, not a constant -- two backward-stable solves of the
            # same least-squares problem differ by O(cond(R1) eps) relative to |phi|, and max |R_kk| / min |R_kk| over the base
            # columns bounds cond(R1) from below; 1e-2 only where near-tolerance pivots (1e-8) sit in the base set.  The
            # comparison with LAPACK on the same rows is in test_full_size_tiago_and_rank_crossing)
            base_d = off["absdiagR"][np.asarray(off["idx_base"])]
            cond_est = base_d.max() / base_d.min()
            phi_tol = min(1e-2, max(1e-9, 4096 * np.finfo(float).eps * cond_est))
            # (phi_b is rounded to 6 decimals, qrdecomposition.py:161: two units of that rounding are the floor)
            assert np.abs(on_["phi_b"] - off["phi_b"]).max() <= max(2e-6, phi_tol * max(1.0, np.abs(off["phi_b"]).max())), (
                cfg, N, seed, cond_est)
            assert abs(on_["residual_norm"] - off["residual_norm"]) <= 1e-9 * off["residual_norm"]
            dep = np.setdiff1d(np.arange(len(off["absdiagR"])), off["idx_base"])
            d_on, d_off = on_["absdiagR"][dep], off["absdiagR"][dep]
            genuine = d_off > TOL_QR / 2
            assert (d_on[~genuine] <= TOL_QR / 2).all(), (cfg, N, seed, d_on[~genuine].max())
            assert np.abs(d_on[genuine] - d_off[genuine]).max(initial=0.0) <= 1e-3 * TOL_QR
            # (the large base pivots behind the first dependent column are not unique -- the direction a dependent column's
            # reflector takes out of the later columns is made of rounding noise, in LAPACK as here -- so they are not
            # compared; the base pivots that could flip a decision, those within 100 x of the tolerance, must agree)
            base = np.asarray(off["idx_base"])
            near = base[off["absdiagR"][base] < 100 * TOL_QR]
            assert np.abs(on_["absdiagR"][near] - off["absdiagR"][near]).max(initial=0.0) <= 1e-3 * TOL_QR
            assert min(on_["absdiagR"][base].min(), off["absdiagR"][base].min()) > TOL_QR
    if cfg == "cfg3_tiago":
        # ... and from OUTSIDE the HIP path: the samples tests/golden/cfg3_tiago_large.json pins at 4e5 (oracle W reduced by a
        # blocked LAPACK Householder TSQR, oracle/pin_cfg3_large.py), rule on AND off against the pinned index sets and the
        # six near-tolerance pivots (four just above TOL_QR, two just below)
        with open(os.path.join(os.path.dirname(__file__), "golden", "cfg3_tiago_large.json")) as f:
            pin4 = {(c["N"], c["seed"]): c for c in json.load(f)["cases"]}[(400_000, 5)]
        q, v, a = sample_inputs(robot.model, 400_000, np.random.default_rng(5), 1.5, 2, 5)
        for on in (False, True):
            pipe = IdentificationPipeline(robot, g.param, params_std=g.params_std(), coupling=g.coupling, w_layout=layout,
                                          null_pivots=on)
            pipe.set_samples(q, v, a)
            pipe.set_tau_from_parameters(g.phi_ref())
            out = pipe.run()
            del pipe
            assert out["idx_e"] == pin4["idx_e"] and out["idx_base"] == pin4["idx_base"], on
            for k, val in pin4["near_tolerance"].items():
                assert abs(out["absdiagR"][int(k)] / val - 1.0) <= 1e-4, (on, k)
            # every other dependent pivot sits far below the tolerance, as in the LAPACK reduction
            dep = np.setdiff1d(np.arange(len(out["absdiagR"])), out["idx_base"] + [int(k) for k in pin4["near_tolerance"]])
            assert out["absdiagR"][dep].max() <= TOL_QR / 2


@pytest.mark.parametrize("flags", [dict(has_friction=True), dict(has_actuator_inertia=True, has_joint_offset=True)])
def test_fused_pass_with_friction_inertia_offset_columns(lib, golden_ur10, oracle_lib, flags):
    """The fused launch with the fv / fs or Ia / off columns switched on (regressor.py:55-70,84-87: the producer's own-link
    columns) -- 61 kept columns + tau, i.e. wider triangles and four consumer waves per workgroup instead of six: W against
    the oracle, the pass against the two-launch pass, and that the fused launch is what ran."""
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    g = golden_ur10
    param = dict(g.param, **flags)
    robot = g.robot()
    params_std = robot.get_standard_parameters(param)
    N = 30000 + 11
    q, v, a, rng, _ = _ur10_problem(g, N, 31)
    W_ref = _oracle_W(g, oracle_lib, q, v, a, param=param)
    phi = rng.uniform(0.1, 1.0, W_ref.shape[1])
    tau = W_ref @ phi + 0.05 * rng.standard_normal(W_ref.shape[0])
    outs = []
    for fuse in (False, True):
        pipe = IdentificationPipeline(robot, param, params_std=params_std, fuse=fuse)
        pipe.set_samples(q, v, a, tau)
        pipe.run()
        out = pipe.run()
        assert pipe.fused_passes == (2 if fuse else 0)
        if fuse:
            W = np.empty((pipe.W.rows, pipe.W.ld))
            lib.check(lib.load().figh_memcpy_d2h(W.ctypes.data, pipe.W.buf.ptr, W.nbytes))
            assert np.abs(W - W_ref).max() <= 1e-12 * np.abs(W_ref).max()
        outs.append(out)
    a_, b_ = outs
    assert len(a_["params_r"]) == 61
    assert a_["idx_e"] == b_["idx_e"] and a_["idx_base"] == b_["idx_base"] and a_["params_base"] == b_["params_base"]
    assert np.abs(a_["col_norm"] - b_["col_norm"]).max() <= 1e-13 * a_["col_norm"].max()
    # (the offset columns next to gravity make one base parameter nearly undetermined -- |phi| ~ 1e5 with random data: the
    # two factorisations agree on it to its conditioning, and to 1e-9 on what the data do determine, the residual)
    assert np.abs(a_["phi_ls"] - b_["phi_ls"]).max() <= 1e-4 * np.abs(a_["phi_ls"]).max()
    assert abs(a_["residual_norm"] - b_["residual_norm"]) <= 1e-9 * a_["residual_norm"]
    ref = (W_ref * W_ref).sum(axis=0)
    assert np.abs(b_["col_norm"] - ref).max() <= 1e-12 * ref.max()


def _synthetic_chain(nj, seed=3):
    """A fixed-base serial chain of ``nj`` revolute joints for the kernels that are instantiated per link count: the UR10
    tree cut after ``nj`` links, or continued with links of random geometry and inertia (flattened form, no URDF)."""
    from figaroh_plus_amd.model import Model
    from figaroh_plus_amd.tools.robot import Robot
    from conftest import ROOT
    flat = Model.from_flat(os.path.join(ROOT, "figaroh_plus_amd", "models", "ur10.json")).to_flat()
    rng = np.random.default_rng(seed)
    n0 = int(flat["njoints"])
    n = nj + 1

    def fit(x, fill):
        x = np.asarray(x)
        if n <= n0:
            return x[:n].copy()
        return np.concatenate([x, np.stack([fill(k) for k in range(n0, n)])])

    def rot(k):
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(-np.pi, np.pi)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
        return np.r_[R.reshape(9), rng.uniform(-0.3, 0.3, 3)]

    def spd(k):
        A = rng.standard_normal((3, 3))
        return (0.01 * (A @ A.T) + 0.005 * np.eye(3)).reshape(9)

    out = dict(flat)
    out["name"], out["njoints"], out["nq"], out["nv"] = "chain%d" % nj, n, nj, nj
    out["names"] = (list(flat["names"]) + ["extra_%d" % k for k in range(n0, n)])[:n]
    out["parents"] = np.arange(-1, n - 1, dtype=np.int32)
    out["parents"][0] = 0
    out["jtype"] = fit(flat["jtype"], lambda k: np.int32(0)).astype(np.int32)
    out["axis"] = fit(flat["axis"], lambda k: np.eye(3)[k % 3])
    out["placement"] = fit(flat["placement"], rot)
    out["idx_q"] = np.r_[0, np.arange(nj)].astype(np.int32)
    out["idx_v"] = np.r_[0, np.arange(nj)].astype(np.int32)
    out["mass"] = fit(flat["mass"], lambda k: rng.uniform(0.5, 3.0))
    out["lever"] = fit(flat["lever"], lambda k: rng.uniform(-0.1, 0.1, 3))
    out["inertia"] = fit(flat["inertia"], spd)
    for key, val in (("lower", -6.28), ("upper", 6.28), ("velocity", 2.0), ("effort", 100.0)):
        out[key] = np.full(nj, val)
    model = Model.from_flat({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in out.items()})
    return Robot("synthetic", None, isFext=False, _model=model)


@pytest.mark.parametrize("nj,flags", [(5, {}), (5, dict(has_friction=True)), (7, {}), (6, dict(has_joint_offset=True))])
def test_fused_pass_other_chains_against_oracle(lib, oracle_lib, nj, flags):
    """The fused launch is instantiated for serial chains of 5, 6 and 7 revolute joints (figh_fused.hip: the stream-out takes
    three or two rows per two passes of the producer wave, the tile buffers 35 - 51 KB): a five-link cut of the UR10 and a
    seven-link continuation with random links, against the oracle's W (1e-12), its column norms, and LAPACK's R of the
    oracle's [W_kept tau] -- index sets and base parameters identical to the two-launch pass on the same samples, which is
    what runs for shapes the launch refuses (eight links: LDS).  Both passes of the fused pipeline are fused."""
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    robot = _synthetic_chain(nj)
    param = dict(is_joint_torques=True, is_external_wrench=False, has_friction=False, has_actuator_inertia=False,
                 has_joint_offset=False, force_torque=None, **{})
    param.update(flags)
    N = 12288 + 29
    rng = np.random.default_rng(40 + nj)
    q, v, a = (rng.uniform(-3, 3, (N, nj)) for _ in range(3))
    om = oracle_lib.OracleModel(robot.model.to_flat())
    mode, fl, ft = oracle_lib.param_flags(param, False)
    W_ref = om.build_regressor_basic(q, v, a, mode, fl, ft)
    assert W_ref.shape == (nj * N, 14 * nj)
    phi = rng.uniform(0.1, 1.0, W_ref.shape[1])
    tau = W_ref @ phi + 0.02 * rng.standard_normal(W_ref.shape[0])
    params_std = robot.get_standard_parameters(param)
    outs = []
    for fuse in (False, True):
        pipe = IdentificationPipeline(robot, param, params_std=params_std, fuse=fuse)
        pipe.set_samples(q, v, a, tau)
        pipe.run()
        lib.check(lib.load().figh_memset(pipe.W.buf.ptr, 0xff, pipe.W.rows * pipe.W.ld * 8))
        out = pipe.run()
        assert pipe.fused_passes == (2 if fuse else 0) and (not fuse or pipe.prefix_passes == 1)
        W = np.empty((pipe.W.rows, pipe.W.ld))
        lib.check(lib.load().figh_memcpy_d2h(W.ctypes.data, pipe.W.buf.ptr, W.nbytes))
        assert np.abs(W - W_ref).max() <= 1e-12 * np.abs(W_ref).max()
        outs.append(out)
    a_, b_ = outs
    ref_norm = (W_ref * W_ref).sum(axis=0)
    assert np.abs(b_["col_norm"] - ref_norm).max() <= 1e-12 * ref_norm.max()
    assert a_["idx_e"] == b_["idx_e"] == np.flatnonzero(ref_norm < 1e-6).tolist()
    assert a_["idx_base"] == b_["idx_base"] and a_["params_base"] == b_["params_base"]
    kept = np.flatnonzero(~(ref_norm < 1e-6))
    assert len(kept) + 1 <= 64
    R_ref = np.linalg.qr(np.c_[W_ref[:, kept], tau], mode="r")
    first_dep = min(set(range(len(kept))) - set(b_["idx_base"]), default=len(kept))
    assert np.abs(b_["absdiagR"][:first_dep] - np.abs(np.diag(R_ref))[:first_dep]).max() <= 1e-10 * np.abs(R_ref).max()
    # the least-squares problem over the BASE columns (qrdecomposition.py:238-244: columns whose pivot is below tol_qr are
    # regrouped, whether exactly dependent or only nearly so) against LAPACK on the oracle's matrix
    Wb = W_ref[:, kept][:, b_["idx_base"]]
    phi_ref, res2 = np.linalg.lstsq(Wb, tau, rcond=None)[:2]
    assert abs(b_["residual_norm"] - np.sqrt(res2[0])) <= 1e-9 * np.sqrt(res2[0])
    assert np.abs(b_["phi_ls"] - phi_ref).max() <= 1e-6 * np.abs(phi_ref).max()
    assert np.abs(a_["phi_ls"] - b_["phi_ls"]).max() <= 1e-6 * np.abs(a_["phi_ls"]).max()


def test_first_pass_is_fused_and_forget_makes_it_first_again(lib, golden_ur10):
    """A script calls the identification functions ONCE (examples/ur10/identification.py:71-83): the very first run() of a
    pipeline learns the kept set from a 4096-sample prefix and runs fused; the result is the golden one.  forget() makes the
    next pass a first pass again (what bench.py reports as ms_first_pass).  A prefix whose kept set is NOT the full one --
    a joint that only starts to move behind the prefix -- is caught by the verification: the pass falls back to the two
    launches, gives the right sets, and the pass after it is fused over the set learnt from them."""
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    g = golden_ur10
    q, v, a, rng, noise = _ur10_problem(g, 50000, 19)
    pipe = IdentificationPipeline(g.robot(), g.param, params_std=g.params_std(), coupling=g.coupling)
    pipe.set_samples(q, v, a)
    pipe.set_tau_from_parameters(g.phi_ref(), noise_std=noise, seed=1)
    out = pipe.run()
    assert pipe.fused_passes == 1 and pipe.prefix_passes == 1
    assert out["idx_e"] == list(g["idx_e"]) and out["idx_base"] == list(g["idx_base"])
    assert out["params_base"] == g.meta["params_base"]
    pipe.run()
    assert pipe.fused_passes == 2 and pipe.prefix_passes == 1
    pipe.forget()
    again = pipe.run()
    assert pipe.fused_passes == 3 and pipe.prefix_passes == 2
    assert again["idx_base"] == out["idx_base"] and np.abs(again["phi_ls"] - out["phi_ls"]).max() <= 1e-10 * np.abs(out["phi_ls"]).max()
    # joints 1 .. 5 at rest and straight for the first 4096 samples: more columns vanish in the prefix than in the whole set
    q2, v2, a2 = q.copy(), v.copy(), a.copy()
    q2[:4096, :5] = 0.0
    v2[:4096, :5] = 0.0
    a2[:4096, :5] = 0.0
    ref = IdentificationPipeline(g.robot(), g.param, params_std=g.params_std(), coupling=g.coupling, fuse=False)
    ref.set_samples(q2, v2, a2)
    ref.set_tau_from_parameters(g.phi_ref(), noise_std=noise, seed=1)
    want = ref.run()
    pipe2 = IdentificationPipeline(g.robot(), g.param, params_std=g.params_std(), coupling=g.coupling)
    pipe2.set_samples(q2, v2, a2)
    pipe2.set_tau_from_parameters(g.phi_ref(), noise_std=noise, seed=1)
    got = pipe2.run()
    assert pipe2.prefix_passes == 1 and pipe2.fused_passes == 0  # the prefix's set was refused by the verification
    assert got["idx_e"] == want["idx_e"] and got["idx_base"] == want["idx_base"] and got["params_base"] == want["params_base"]
    got = pipe2.run()
    assert pipe2.fused_passes == 1 and got["idx_base"] == want["idx_base"]


def test_fused_pass_triangle_against_lapack(lib, golden_ur10, oracle_lib):
    """The plain triangle of the fused launch (tol_qr < 0) against LAPACK's R of the oracle's [W_e tau]: R^T R to 1e-12."""
    g = golden_ur10
    N = 8192 + 17
    q, v, a, rng, _ = _ur10_problem(g, N, 5)
    W_ref = _oracle_W(g, oracle_lib, q, v, a)
    tau = rng.standard_normal(6 * N)
    kept = np.array([c for c in range(84) if c not in set(int(x) for x in g["idx_e"])], dtype=np.int32)
    n, nc = len(kept), len(kept) + 1
    from figaroh_plus_amd.tools.regressor import _samples_to_device
    robot = g.robot()
    _, d_q, d_v, d_a = _samples_to_device(robot.model, q, v, a)
    d_W = lib.DeviceArray((6 * N * 84,), np.float64)
    d_cs = lib.DeviceArray((84,), np.float64)
    d_kept = lib.DeviceArray.from_host(kept)
    d_tau = lib.DeviceArray.from_host(tau)
    d_R = lib.DeviceArray((nc * nc,), np.float64)
    assert lib.regressor_tsqr_fused(robot.device_model(), 0, N, d_q, d_v, d_a, d_W, 84, d_cs, d_kept, n, d_tau, -1.0, d_R)
    R = d_R.to_host().reshape(nc, nc)
    W = d_W.to_host().reshape(6 * N, 84)
    assert np.abs(W - W_ref).max() <= 1e-12 * np.abs(W_ref).max()
    # zero pattern: on these random samples the closed-form rows leave residues of 1e-15 in three columns of link 2 where
    # the oracle's literal propagation cancels exactly (the two-launch kernel does the same); nothing larger than that
    assert np.abs(W[W_ref == 0]).max(initial=0.0) <= 1e-14 * np.abs(W_ref).max()
    assert np.abs(W_ref[W == 0]).max(initial=0.0) <= 1e-14 * np.abs(W_ref).max()
    A = np.c_[W_ref[:, kept], tau]
    G = A.T @ A
    assert np.abs(R.T @ R - G).max() <= 1e-12 * np.abs(G).max()
    assert np.abs(np.tril(R, -1)).max() == 0.0
    cs = d_cs.to_host()
    ref = (W_ref * W_ref).sum(axis=0)
    assert np.abs(cs - ref).max() <= 1e-13 * ref.max()
    # unsupported shapes answer without launching anything
    assert not lib.regressor_tsqr_fused(robot.device_model(), 0, 1000, d_q, d_v, d_a, d_W, 84, d_cs, d_kept, n, d_tau, -1.0, d_R)


# ------------------------------------------------------------------------------------------------ device-resident WLS
def test_pipeline_wls_matches_golden(lib, golden):
    """IdentificationPipeline.run(wls=True) on the golden samples against what the reference's script statements
    (examples/staubli_TX40/identification.py:305-346, run by oracle/gen_golden.py on the reference's own W_b) produce:
    phi to the 6-decimal rounding, std% to the 2-decimal rounding."""
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    g = golden
    if "phi_wls_script" not in g.z.files:
        pytest.skip("no WLS golden")
    for layout in ("dense", "block-compact"):
        pipe = IdentificationPipeline(g.robot(), g.param, params_std=g.params_std(), coupling=g.coupling, w_layout=layout)
        pipe.set_samples(g["q_big"], g["v_big"], g["a_big"], g["tau"])
        out = pipe.run(wls=True)
        assert out["idx_base"] == list(g["idx_base"])
        assert np.abs(out["phi_wls"] - g["phi_wls_script"]).max() <= 1.5e-6 * max(1.0, np.abs(g["phi_wls_script"]).max())
        big = np.abs(g["std_wls_script"]) < 1e4
        assert np.abs(out["std_wls"] - g["std_wls_script"])[big].max() <= 0.011 + 1e-5 * np.abs(g["std_wls_script"][big]).max()
        out2 = pipe.run(wls=True)  # (second pass: the fused launch where it applies)
        assert np.abs(out2["phi_wls"] - out["phi_wls"]).max() <= 1e-6 * max(1.0, np.abs(out["phi_wls"]).max())


@pytest.mark.parametrize("cfg,N,layout", [("cfg3_tiago", 20000, "block-compact"), ("cfg3_tiago", 20000, "dense"),
                                         ("cfg2_ur10", 100000, "dense"), ("cfg4_talos", 20000, "dense")])
def test_pipeline_wls_against_oracle_formula(lib, oracle_lib, cfg, N, layout):
    """The device-resident WLS at a size where the oracle's W fits the host: per-joint variances, phi and std% against
    oracle_np.wls_script (the script's statements without the dense SIGMA) on the oracle's own W_b -- phi to 1e-6
    relative (north_star tolerance), std% to the 2-decimal rounding.  TIAGo goes through the per-row-block triangles (W is
    not read again), the others through the second pass over W."""
    from conftest import Golden
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    g = Golden(cfg)
    robot = g.robot()
    rng = np.random.default_rng(404)
    if cfg == "cfg2_ur10":
        q, v, a = (rng.uniform(-6, 6, (N, 6)) for _ in range(3))
    else:
        q, v, a = sample_inputs(robot.model, N, rng, 1.5, 2, 5)
    W = _oracle_W(g, oracle_lib, q, v, a)
    nblk = W.shape[0] // N
    # joint-dependent noise: the weights matter
    tau = W @ g.phi_ref() + rng.standard_normal(W.shape[0]) * np.repeat(0.02 * (1.0 + np.arange(nblk)), N)
    pipe = IdentificationPipeline(robot, g.param, params_std=g.params_std(), coupling=g.coupling, w_layout=layout)
    pipe.set_samples(q, v, a, tau)
    out = pipe.run(wls=True)
    out = pipe.run(wls=True)
    kept = [i for i in range(W.shape[1]) if i not in set(out["idx_e"])]
    W_b = W[:, kept][:, out["idx_base"]]
    del W
    phi_ref, std_ref = oracle_np.wls_script(W_b, tau, out["phi_b"], [N] * nblk)
    sig2_ref = np.array([np.sum((tau[b * N:(b + 1) * N] - W_b[b * N:(b + 1) * N] @ out["phi_b"]) ** 2) / N for b in range(nblk)])
    assert np.abs(out["sigma2_joint"] - sig2_ref).max() <= 1e-9 * sig2_ref.max()
    assert np.abs(out["phi_wls"] - phi_ref).max() <= 1e-6 * np.abs(phi_ref).max() + 1e-6  # (both rounded to 6 decimals)
    # estimates that round to exactly zero have std% = inf on both sides (the script's division by zero; asserted, not masked)
    zero = out["phi_wls"] == 0.0
    assert np.array_equal(zero, phi_ref == 0.0) or np.abs(out["phi_wls"] - phi_ref)[zero ^ (phi_ref == 0.0)].max() <= 1e-6
    both = zero & (phi_ref == 0.0)
    assert np.isinf(out["std_wls"][zero]).all() and np.isinf(std_ref[both]).all()
    ok = ~zero & (phi_ref != 0.0) & (np.abs(std_ref) < 1e4)
    assert np.abs(out["std_wls"][ok] - std_ref[ok]).max() <= 0.011 + 1e-5 * np.abs(std_ref[ok]).max()
    if cfg == "cfg3_tiago" and layout == "block-compact":
        assert out["wls_source"] == "per-row-block triangles"


# ------------------------------------------------------------------------------------------------ real-data chain in HBM
def test_tx40_real_data_device_resident_chain(lib, monkeypatch):
    """The known-answer replay of test_tx40_real_data_known_answers_hip with the regressor RESIDENT in HBM from K1 to
    double_QR: regressor (TX40 coupling columns fused) -> two decimate-by-10 stages -> zero-velocity row rejection (device
    stream compaction) -> elimination -> double_QR -> sigma -> OLS -> WLS -> essential-parameter loop.  GpuMatrix.numpy is
    disabled while the chain runs: no copy of W (or of a derived matrix) to the host can happen unnoticed."""
    from tx40_real_common import load_fixture, trajectories, tx40
    from figaroh_plus_amd.device import GpuMatrix
    from figaroh_plus_amd.identification.identification_tools import (decimate_joint_blocks, essential_parameters,
                                                                       least_squares, low_pass_filter_data, reject_rows,
                                                                       relative_stdev, weighted_least_squares_blocks)
    from figaroh_plus_amd.tools.qrdecomposition import double_QR, rfactor
    from figaroh_plus_amd.tools.regressor import _samples_to_device, build_regressor_device, eliminate_non_dynaffect
    z, meta = load_fixture()
    g, robot, param, params_std = tx40()
    q, dq, ddq, tau = trajectories(z, robot, param, low_pass_filter_data)
    N, d_q, d_v, d_a = _samples_to_device(robot.model, q, dq, ddq)
    W, _ = build_regressor_device(robot, d_q, d_v, d_a, N, param, coupling=True)
    assert isinstance(W, GpuMatrix) and W.shape == (6 * N, 87)

    def no_copy(self, *a, **k):
        raise AssertionError("the regressor was copied to the host inside the device-resident chain")
    monkeypatch.setattr(GpuMatrix, "numpy", no_copy)
    monkeypatch.setattr(GpuMatrix, "__array__", no_copy)
    nj = tau.shape[0] // 6
    W_head = GpuMatrix(W.buf, 6 * nj, W.cols, W.ld)  # the scripts cut W's joint blocks with tau's block length
    W_list, tau_list = decimate_joint_blocks(W_head, tau, 6, q=10, stages=2)
    W_, tau_, counts = reject_rows(W_list, tau_list, [i * 14 + 11 for i in range(6)], param["dq_lim_def"][:6])
    assert counts == list(z["counts"]) and isinstance(W_, GpuMatrix)
    W_e, params_r = eliminate_non_dynaffect(W_, params_std, 0.001)
    assert isinstance(W_e, GpuMatrix) and params_r == meta["params_r"]
    W_b, base_parameters, params_base, phi_b = double_QR(tau_, W_e, params_r)
    assert isinstance(W_b, GpuMatrix) and params_base == meta["csv_expressions"]
    csvv = z["csv"]
    assert np.abs(phi_b - z["phi_b"]).max() <= 1.5e-6 and np.abs(phi_b - csvv[:, 0]).max() <= 4e-4
    std = relative_stdev(W_b, phi_b, tau_)
    assert np.abs(std - z["std_ols"]).max() <= 0.011 + 1e-4 * np.abs(z["std_ols"]).max()
    phi_ols = np.around(least_squares(W_b, tau_), 6)
    assert np.abs(phi_ols - z["phi_ols"]).max() <= 1.5e-6
    phi_w, std_w, det = weighted_least_squares_blocks(W_b, tau_, phi_b, counts, return_details=True)
    assert np.abs(phi_w - z["phi_wls"]).max() <= 1.5e-6 and np.abs(phi_w - csvv[:, 2]).max() <= 4e-4
    ok = z["std_wls"] < 1e3
    assert (np.abs(std_w - z["std_wls"])[ok] / z["std_wls"][ok]).max() <= 2e-3
    # the essential-parameter loop on the two triangles of [W_b tau] (examples/staubli_TX40/identification.py:354-399)
    R_ols = rfactor(W_b, tau=tau_)
    ess = essential_parameters(R_ols, det["R_wls"], list(params_base), std_w, param["ratio_essential"], rows_total=W_b.rows)
    monkeypatch.undo()
    # ... against the script's loop on the host copy of the same W_b
    Wb_h, tau_h = W_b.numpy(), tau_.to_host()[:W_b.rows]
    ref = oracle_np.essential_script(Wb_h, tau_h, list(params_base), std_w, det["sigma2_joint"], counts,
                                     param["ratio_essential"])
    assert ess["iterations"] == ref["iterations"] and ess["params_essential"] == ref["params_essential"]
    if ref["iterations"]:
        assert np.abs(ess["phi_e_wls"] - ref["phi_e_wls"]).max() <= 1.5e-6
        assert np.abs(ess["phi_e_ols"] - ref["phi_e_ols"]).max() <= 1.5e-6
        fin = np.isfinite(ref["std_e_wls"]) & (np.abs(ref["std_e_wls"]) < 1e3)
        assert np.abs(ess["std_e_wls"] - ref["std_e_wls"])[fin].max() <= 0.011 + 2e-3 * np.abs(ref["std_e_wls"][fin]).max()


@pytest.mark.parametrize("rows,cols,ld", [(1, 3, 3), (63, 5, 8), (64, 87, 87), (65, 87, 90), (4496, 87, 87), (20011, 14, 16)])
def test_compact_rows_matches_numpy(lib, rows, cols, ld):
    from figaroh_plus_amd.device import GpuMatrix
    rng = np.random.default_rng(rows + cols)
    W = rng.standard_normal((rows, ld))
    tau = rng.standard_normal(rows)
    key, thr = cols // 2, 0.6
    dW = GpuMatrix(lib.DeviceArray.from_host(W.reshape(-1)), rows, cols, ld)
    d_tau = lib.DeviceArray.from_host(tau)
    out = GpuMatrix.empty(rows, cols)
    d_to = lib.DeviceArray((rows,), np.float64)
    kept = lib.compact_rows(dW.ptr, rows, cols, ld, d_tau.ptr, key, thr, out.ptr, cols, d_to.ptr)
    keep = np.abs(W[:, key]) >= thr
    assert kept == int(keep.sum())
    assert np.array_equal(out.numpy()[:kept], W[keep][:, :cols]) and np.array_equal(d_to.to_host()[:kept], tau[keep])


# ------------------------------------------------------------------------------------------------ 8f-1 active joints (TIAGo)
def _tiago_active():
    from conftest import GOLD, Golden
    with open(os.path.join(GOLD, "tiago_active.json")) as f:
        meta = json.load(f)
    return Golden("cfg3_tiago"), meta, np.load(os.path.join(GOLD, "tiago_active.npz"))


def test_tiago_active_joint_decimation_matches_reference_script(lib):
    """examples/tiago/identification.py:142-187, :319-337 with the drop-in functions: full regressor, elimination at 1e-3 on
    the norms of the FULL matrix, decimation (q = 10, one stage) of the eight ACTIVE row blocks only
    (decimate_joint_blocks(..., blocks=act_idxv)), double_QR on their stack -- against the fixture produced by the reference's
    own decimate_data / double_QR / relative_stdev (oracle/gen_golden_tiago_active.py): identical idx_e, params_r and
    base-parameter expressions, the decimated stack to 1e-9 of its scale, phi_b to the 6-decimal rounding."""
    from figaroh_plus_amd.identification.identification_tools import decimate_joint_blocks, relative_stdev
    from figaroh_plus_amd.tools.qrdecomposition import double_QR
    from figaroh_plus_amd.tools.regressor import build_regressor_basic, build_regressor_reduced, get_index_eliminate
    g, meta, z = _tiago_active()
    robot = g.robot()
    act = meta["act_idxv"]
    q, v, a, tau = z["dec_q"], z["dec_v"], z["dec_a"], z["dec_tau"]
    N = len(q)
    params_std = g.params_std()
    W = build_regressor_basic(robot, q, v, a, g.param)
    idx_e, params_r = get_index_eliminate(W, params_std, tol_e=meta["tol_e"])
    assert list(idx_e) == z["dec_idx_e"].tolist() and list(params_r) == meta["dec"]["params_r"]
    W_e = build_regressor_reduced(W, idx_e)
    W_list, tau_list = decimate_joint_blocks(W_e, tau.T.reshape(-1), len(act), q=10, stages=1, blocks=act)
    W_rf, tau_rf = np.vstack(W_list), np.concatenate(tau_list)
    assert W_rf.shape[0] == int(z["dec_rows"][0]) and W_rf.shape[1] == len(params_r)
    assert np.abs(tau_rf - z["dec_tau_rf"]).max() <= 1e-9 * np.abs(z["dec_tau_rf"]).max()
    assert np.abs(W_rf[::7] - z["dec_W_rf_rows"]).max() <= 1e-9 * np.abs(z["dec_W_rf_rows"]).max()
    colsq = np.einsum("ij,ij->j", W_rf, W_rf)
    assert np.abs(colsq - z["dec_W_rf_colsq"]).max() <= 1e-9 * z["dec_W_rf_colsq"].max()
    W_b, bp, params_base, phi_b, phi_std = double_QR(tau_rf, W_rf, params_r, params_std)
    assert list(params_base) == meta["dec"]["params_base"]
    assert np.abs(phi_b - z["dec_phi_b"]).max() <= 2e-6 and np.abs(phi_std - z["dec_phi_std"]).max() <= 2e-5
    std = relative_stdev(W_b, phi_b, tau_rf)
    fin = np.isfinite(z["dec_std"]) & (np.abs(z["dec_std"]) < 1e4)
    assert np.abs(std - z["dec_std"])[fin].max() <= 0.011 + 1e-4 * np.abs(z["dec_std"][fin]).max()
    # the device-resident form gives the same blocks
    from figaroh_plus_amd.device import to_device
    Wd, _ = to_device(W_e)
    Wl_d, tl_d = decimate_joint_blocks(Wd, tau.T.reshape(-1), len(act), q=10, stages=1, blocks=act)
    for i in range(len(act)):
        assert np.array_equal(Wl_d[i].numpy(), W_list[i])
    with pytest.raises(ValueError):
        decimate_joint_blocks(W_e, tau.T.reshape(-1), len(act), q=10, stages=1, blocks=act[:-1])


@pytest.mark.parametrize("layout", ["block-compact", "dense"])
def test_pipeline_active_row_blocks(lib, oracle_lib, layout):
    """IdentificationPipeline(row_blocks=act_idxv): (i) on the fixture's ``raw`` case -- the script with decimate=False on the
    active blocks, produced by the reference's double_QR -- identical idx_e (tol_e 1e-3 on the FULL regressor's norms),
    params_r, expressions; phi_b to the rounding; (ii) at 50 000 samples against LAPACK on the oracle's stacked active
    blocks; (iii) only the active blocks are stored: block-compact W takes 16 N sum_{active} |subtree_j| doubles."""
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    g, meta, z = _tiago_active()
    robot = g.robot()
    act = meta["act_idxv"]
    q, v, a, tau = z["raw_q"], z["raw_v"], z["raw_a"], z["raw_tau"]
    pipe = IdentificationPipeline(robot, g.param, params_std=g.params_std(), tol_e=meta["tol_e"], row_blocks=act,
                                  w_layout=layout)
    pipe.set_samples(q, v, a, tau.T.reshape(-1))
    out = pipe.run()
    out = pipe.run(wls=True)
    assert out["idx_e"] == z["raw_idx_e"].tolist() and out["params_r"] == meta["raw"]["params_r"]
    assert out["idx_base"] == z["raw_idx_base"].tolist() and out["params_base"] == meta["raw"]["params_base"]
    assert np.abs(out["phi_b"] - z["raw_phi_b"]).max() <= 2e-6
    assert out["rows"] == len(act) * len(q) and len(out["sigma2_joint"]) == len(act)
    if layout == "block-compact":
        sizes = pipe._subtree_sizes()
        assert pipe.W.buf.size == 16 * len(q) * int(sizes[act].sum())
    with pytest.raises(ValueError):
        pipe.set_samples(q, v, a, np.zeros(24 * len(q)))  # tau of ALL dofs: not what a pipeline with row_blocks takes
    # (ii) a size the fixtures do not reach
    N = 50000
    rng = np.random.default_rng(77)
    q, v, a = sample_inputs(robot.model, N, rng, 1.5, 2, 5)
    W = _oracle_W(g, oracle_lib, q, v, a)
    norms = np.einsum("ij,ij->j", W, W)
    kept = np.flatnonzero(~(norms < 1e-6))
    Wa = np.vstack([W[b * N:(b + 1) * N][:, kept] for b in act])
    del W
    tau = Wa @ g.phi_ref()[kept] + 0.05 * rng.standard_normal(Wa.shape[0])
    pipe = IdentificationPipeline(robot, g.param, params_std=g.params_std(), row_blocks=act, w_layout=layout)
    pipe.set_samples(q, v, a, tau)
    pipe.run()
    out = pipe.run()
    assert out["idx_e"] == np.flatnonzero(norms < 1e-6).tolist()
    R = np.linalg.qr(Wa, mode="r")
    base = np.flatnonzero(np.abs(np.diag(R)) > 1e-8).tolist()
    assert out["idx_base"] == base
    phi_ref, res2 = np.linalg.lstsq(Wa[:, base], tau, rcond=None)[:2]
    assert abs(out["residual_norm"] - np.sqrt(res2[0])) <= 1e-9 * np.sqrt(res2[0])
    assert np.abs(out["phi_ls"] - phi_ref).max() <= 1e-6 * np.abs(phi_ref).max()


def test_tiago_real_data_known_answers_hip(lib):
    """The TIAGo known-answer replay (tests/test_oracle.py::test_tiago_real_data_known_answers) through the HIP path: the tree
    kernel's regressor of the 5 870 real samples, the elimination, the active-joint decimation on the device and double_QR
    reproduce the 44 expressions of the reference's committed, Pinocchio-produced tiago_bp_19_Oct_2024_2320.csv verbatim, its
    values to the 6-decimal rounding and its standard deviations to their 2 decimals."""
    from figaroh_plus_amd.identification.identification_tools import decimate_joint_blocks, relative_stdev
    from figaroh_plus_amd.tools.qrdecomposition import double_QR
    from figaroh_plus_amd.tools.regressor import build_regressor_basic, build_regressor_reduced, get_index_eliminate
    from tiago_real_common import load_fixture, tiago, trajectories
    z, meta = load_fixture()
    g, robot, param, params_std = tiago()
    p, v, a, tau = trajectories(z, meta, robot)
    W = build_regressor_basic(robot, p, v, a, param)
    chk = np.array([W.sum(), np.abs(W).sum(), (W * W).sum()])
    assert np.abs(chk - z["W_checksum"]).max() <= 1e-11 * np.abs(z["W_checksum"]).max()
    idx_e, params_r = get_index_eliminate(W, params_std, tol_e=meta["tol_e"])
    assert list(idx_e) == z["idx_e"].tolist() and list(params_r) == meta["params_r"]
    W_e = build_regressor_reduced(W, idx_e)
    act = meta["act_idxv"]
    W_list, tau_list = decimate_joint_blocks(W_e, tau.T.reshape(-1), len(act), q=10, stages=1, blocks=act)
    W_rf, tau_rf = np.vstack(W_list), np.concatenate(tau_list)
    assert np.abs(tau_rf - z["tau_rf"]).max() <= 1e-12 * np.abs(tau_rf).max()
    assert np.abs(W_rf[::29] - z["W_rf_rows"]).max() <= 1e-10 * np.abs(W_rf).max()
    W_b, bp, params_base, phi_b, phi_std = double_QR(tau_rf, W_rf, params_r, params_std)
    assert list(params_base) == meta["csv_expressions"]
    csvv = z["csv"]
    assert np.abs(phi_b - csvv[:, 0]).max() <= 2e-6
    assert np.abs(phi_std - z["phi_std"]).max() <= 2e-5
    std = relative_stdev(W_b, phi_b, tau_rf)
    assert np.abs(std - csvv[:, 1] / 100).max() <= 0.011


def _synthetic_tree(parents, seed=5, massless=(), freeflyer=False):
    """A tree of single-dof joints (revolute / prismatic / continuous at random, random unit axes, placements and inertias;
    ``massless`` links carry no body) from a parent list in depth-first numbering: parents[k - 1] = parent of joint k.
    ``freeflyer``: joint 1 is a free-flyer root with a body (parents[0] is ignored), the model of an external-wrench regressor."""
    from figaroh_plus_amd.model import Inertia, Model, SE3
    from figaroh_plus_amd.tools.robot import Robot
    rng = np.random.default_rng(seed)
    model = Model("tree%d" % len(parents))
    for k, par in enumerate(parents, start=1):
        if freeflyer and k == 1:
            model.add_joint(0, 3, None, SE3(), "root_joint")
            A = rng.standard_normal((3, 3))
            model.append_body(1, Inertia(rng.uniform(2.0, 5.0), rng.uniform(-0.1, 0.1, 3), 0.02 * (A @ A.T) + 0.01 * np.eye(3)), SE3())
            continue
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        w = rng.standard_normal(3)
        w /= np.linalg.norm(w)
        ang = rng.uniform(-np.pi, np.pi)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
        jid = model.add_joint(par, int(rng.choice([0, 0, 1, 2])), axis, SE3(R, rng.uniform(-0.3, 0.3, 3)), "j%d" % k,
                              limits=(-3.0, 3.0, 2.0, 50.0))
        assert jid == k
        if k not in massless:
            A = rng.standard_normal((3, 3))
            model.append_body(k, Inertia(rng.uniform(0.5, 3.0), rng.uniform(-0.1, 0.1, 3), 0.01 * (A @ A.T) + 0.005 * np.eye(3)),
                              SE3())
    return Robot("synthetic", None, isFext=freeflyer, _model=model)


_TREES = {
    # a chain deeper than two windows of row slots; a complete binary tree; a spine with a leaf at every vertebra; a star of
    # short chains; one long and one short branch under a common trunk with a massless link in the middle
    "chain13": list(range(0, 13)),
    "binary15": [0, 1, 2, 3, 3, 2, 6, 6, 1, 9, 10, 10, 9, 13, 13],
    "caterpillar": [0, 1, 1, 3, 3, 5, 5, 7, 7, 9, 9, 11, 11, 13],
    "star": [0, 1, 2, 0, 4, 5, 0, 7, 0, 0, 10, 11, 12],
    "fork": [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 3, 11, 1],
}


@pytest.mark.parametrize("shape", sorted(_TREES))
@pytest.mark.parametrize("flags", [{}, dict(has_friction=True, has_actuator_inertia=True, has_joint_offset=True)])
def test_tree_walks_random_trees_against_oracle(lib, oracle_lib, shape, flags):
    """The joint-torque walks of the tape kernel (figh_regressor_tree.hip, build_tape_torque_rows: one walk serves the row
    blocks of up to kRowSlots levels of joints, axes carried in slots, branches re-entered from the root) on random trees of
    every shape the windowing distinguishes, against the C oracle: the dense W (the reference's layout) to 1e-12, the
    block-compact W of the pipeline through its spot rows and column norms, and a subset of active row blocks."""
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from figaroh_plus_amd.tools.regressor import build_regressor_basic
    parents = _TREES[shape]
    robot = _synthetic_tree(parents, seed=len(parents), massless=(4,) if shape == "fork" else ())
    m = robot.model
    param = dict(is_joint_torques=True, is_external_wrench=False, has_friction=False, has_actuator_inertia=False,
                 has_joint_offset=False, force_torque=None)
    param.update(flags)
    N = 64 * 3 + 17
    rng = np.random.default_rng(7 + len(parents))
    q = np.zeros((N, m.nq))
    for j in m.joints[1:]:
        if j.nq == 2:
            th = rng.uniform(-3, 3, N)
            q[:, j.idx_q], q[:, j.idx_q + 1] = np.cos(th), np.sin(th)
        else:
            q[:, j.idx_q] = rng.uniform(-2, 2, N)
    v, a = rng.uniform(-2, 2, (N, m.nv)), rng.uniform(-3, 3, (N, m.nv))
    om = oracle_lib.OracleModel(m.to_flat())
    mode, fl, ft = oracle_lib.param_flags(param, False)
    W_ref = om.build_regressor_basic(q, v, a, mode, fl, ft)
    scale = np.abs(W_ref).max()
    W = build_regressor_basic(robot, q, v, a, param)
    assert W.shape == W_ref.shape == (m.nv * N, 14 * m.nv)
    assert np.abs(W - W_ref).max() <= 1e-12 * scale
    # the pipeline's layouts: link-padded (16 columns per link), block-compact (row block j = its subtree's window), and the
    # block-compact layout of every other row block (the others are walked for the column norms only)
    params_std = robot.get_standard_parameters(param)
    nl = m.njoints - 1
    tau = W_ref @ np.array(list(params_std.values()), dtype=float) + 1e-3 * rng.standard_normal(len(W_ref))
    ref_sq = (W_ref * W_ref).sum(axis=0)
    padded = np.zeros((len(W_ref), 16 * nl))
    padded[:, (np.arange(14 * nl) // 14) * 16 + np.arange(14 * nl) % 14] = W_ref
    sub_end = []
    for j in range(1, m.njoints):
        e = j + 1
        while e < m.njoints:
            k = e
            while k > j:
                k = m.parents[k]
            if k != j:
                break
            e += 1
        sub_end.append(e)
    for layout, blocks in (("link-padded", None), ("block-compact", None), ("block-compact", list(range(0, m.nv, 2)))):
        pipe = IdentificationPipeline(robot, param, params_std=params_std, row_blocks=blocks, w_layout=layout)
        t = tau if blocks is None else np.concatenate([tau[b * N:(b + 1) * N] for b in blocks])
        pipe.set_samples(q, v, a, t)
        out = pipe.run()
        out = pipe.run()
        assert np.abs(out["col_norm"] - ref_sq).max() <= 1e-12 * ref_sq.max()
        if layout == "link-padded":
            assert np.abs(pipe.W.numpy() - padded).max() <= 1e-12 * scale
        else:
            comp = pipe.W.buf.to_host()
            off, ld = pipe._compact
            for row in range(m.nv):
                j = int(np.flatnonzero(np.array([jm.idx_v for jm in m.joints[1:]]) == row)[0]) + 1
                if blocks is not None and row not in blocks:
                    assert ld[row] == 0
                    continue
                assert ld[row] == 16 * (sub_end[j - 1] - j)
                blk = comp[off[row]:off[row] + N * ld[row]].reshape(N, ld[row])
                assert np.abs(blk - padded[row * N:(row + 1) * N, 16 * (j - 1):16 * (j - 1) + ld[row]]).max() <= 1e-12 * scale
        keep = [c for c in range(W_ref.shape[1]) if c not in set(out["idx_e"])]
        Wk = W_ref[:, keep] if blocks is None else np.vstack([W_ref[b * N:(b + 1) * N, keep] for b in blocks])
        res = Wk @ np.linalg.lstsq(Wk, t, rcond=None)[0] - t
        assert abs(out["residual_norm"] - np.linalg.norm(res)) <= 1e-8 * max(1.0, np.linalg.norm(t))


@pytest.mark.parametrize("shape", ["binary15", "caterpillar", "star", "fork"])
def test_freeflyer_walk_state_copy_on_random_trees(lib, oracle_lib, shape):
    """The free-flyer walk of the tape kernel with the state copy at branch joints (STEP_SAVE / OP_RESTORE: the force-compact
    instantiation, the pipeline's default layout for an external-wrench regressor) on random floating-base trees with nested
    and sibling branch joints: column norms against the oracle's W, and every result of the pass equal to that of the
    link-padded layout (the instantiation without the copy: every branch is re-entered from the root), whose W is compared
    with the oracle entry by entry."""
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    parents = [0] + [p + 1 for p in _TREES[shape]]  # the tree hangs off the free-flyer root
    massless = (6, 9) if shape in ("fork", "caterpillar") else ()
    robot = _synthetic_tree(parents, seed=3 + len(parents), massless=massless, freeflyer=True)
    m = robot.model
    param = dict(is_joint_torques=False, is_external_wrench=True, has_friction=False, has_actuator_inertia=False,
                 has_joint_offset=False, force_torque=["All"])
    N = 64 * 40 + 23  # (the force / torque split of the force-compact layout wants 32 rows per kept column)
    rng = np.random.default_rng(11 + len(parents))
    q = np.zeros((N, m.nq))
    quat = rng.standard_normal((N, 4))
    q[:, :3], q[:, 3:7] = rng.uniform(-1, 1, (N, 3)), quat / np.linalg.norm(quat, axis=1)[:, None]
    for j in m.joints[2:]:
        if j.nq == 2:
            th = rng.uniform(-3, 3, N)
            q[:, j.idx_q], q[:, j.idx_q + 1] = np.cos(th), np.sin(th)
        else:
            q[:, j.idx_q] = rng.uniform(-2, 2, N)
    v, a = rng.uniform(-2, 2, (N, m.nv)), rng.uniform(-3, 3, (N, m.nv))
    om = oracle_lib.OracleModel(m.to_flat())
    mode, fl, ft = oracle_lib.param_flags(param, False)
    W_ref = om.build_regressor_basic(q, v, a, mode, fl, ft)
    nl = m.njoints - 1
    assert W_ref.shape == (6 * N, 14 * nl)
    scale = np.abs(W_ref).max()
    params_std = robot.get_standard_parameters(param)
    tau = W_ref @ np.array(list(params_std.values()), dtype=float) + 1e-3 * rng.standard_normal(len(W_ref))
    ref_sq = (W_ref * W_ref).sum(axis=0)
    outs = {}
    for layout in ("link-padded", "dense"):
        pipe = IdentificationPipeline(robot, param, params_std=params_std, w_layout=layout)
        pipe.set_samples(q, v, a, tau)
        pipe.run()
        outs[layout] = pipe.run()
        assert np.abs(outs[layout]["col_norm"] - ref_sq).max() <= 1e-12 * ref_sq.max()
        if layout == "link-padded":
            assert not getattr(pipe, "_force_ld", 0)
            padded = np.zeros((len(W_ref), 16 * nl))
            padded[:, (np.arange(14 * nl) // 14) * 16 + np.arange(14 * nl) % 14] = W_ref
            assert np.abs(pipe.W.numpy() - padded).max() <= 1e-12 * scale
        else:
            assert getattr(pipe, "_force_ld", 0) > 0  # (the instantiation with the state copy ran)
    a_, b_ = outs["link-padded"], outs["dense"]
    assert a_["idx_e"] == b_["idx_e"] and a_["idx_base"] == b_["idx_base"] and a_["params_base"] == b_["params_base"]
    assert np.abs(a_["col_norm"] - b_["col_norm"]).max() <= 1e-13 * ref_sq.max()
    assert abs(a_["residual_norm"] - b_["residual_norm"]) <= 1e-9 * max(1.0, a_["residual_norm"])
    assert np.abs(a_["phi_ls"] - b_["phi_ls"]).max() <= 1e-6 * max(1.0, np.abs(a_["phi_ls"]).max())


def _random_parents(rng, n, deep=0.6):
    """A random tree of n joints in depth-first numbering: the parent of joint k is a joint on the root path of joint k - 1
    (or the universe) -- with probability ``deep`` joint k - 1 itself, which makes long chains with side branches."""
    parents, path = [0], [1]
    for k in range(2, n + 1):
        if rng.random() < deep:
            par = path[-1]
        else:
            par = int(rng.choice([0] + path))
        path = path[:path.index(par) + 1] if par else []
        path.append(k)
        parents.append(par)
    return parents


@pytest.mark.parametrize("seed", [131, 208])
def test_null_rule_certificate_falls_back_on_ill_conditioned_trees(lib, oracle_lib, seed):
    """Two random floating-base trees that tools/fuzz_trees.py found in round 6 (250 seeds): cond(W_b) ~ 1e14 .. 1e16, regrouping
    coefficients in the hundreds -- the null-pivot rule, which perturbs a column by at most tol_qr / 64, turned that into a
    SPURIOUS base parameter (pivot 1.2e-8 resp. 1.1e-7 where plain Householder and LAPACK see a dependent column).  The
    pipeline certifies every pass that ran under the rule (_host.null_rule_certified) and repeats an uncertified one without
    it: default settings must return the index sets of the plain factorisation, which are LAPACK's on the oracle's W."""
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from figaroh_plus_amd.tools.qrdecomposition import TOL_QR, get_baseIndex
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(8, 31))
    parents = _random_parents(rng, n, deep=float(rng.choice([0.4, 0.6, 0.8])))
    massless = tuple(int(k) for k in rng.choice(np.arange(2, n + 1), size=n // 6, replace=False))
    robot = _synthetic_tree([0] + [p + 1 for p in parents], seed=seed, massless=tuple(k + 1 for k in massless), freeflyer=True)
    m = robot.model
    param = dict(is_joint_torques=False, is_external_wrench=True, has_friction=False, has_actuator_inertia=False,
                 has_joint_offset=False, force_torque=["All"])
    N = 64 * 90 + 17
    q = np.zeros((N, m.nq))
    quat = rng.standard_normal((N, 4))
    q[:, :3], q[:, 3:7] = rng.uniform(-1, 1, (N, 3)), quat / np.linalg.norm(quat, axis=1)[:, None]
    for j in m.joints[2:]:
        if j.nq == 2:
            th = rng.uniform(-3, 3, N)
            q[:, j.idx_q], q[:, j.idx_q + 1] = np.cos(th), np.sin(th)
        else:
            q[:, j.idx_q] = rng.uniform(-2, 2, N)
    v, a = rng.uniform(-2, 2, (N, m.nv)), rng.uniform(-3, 3, (N, m.nv))
    mode, fl, ft = oracle_lib.param_flags(param, False)
    W_ref = oracle_lib.OracleModel(m.to_flat()).build_regressor_basic(q, v, a, mode, fl, ft)
    params_std = robot.get_standard_parameters(param)
    tau = W_ref @ np.array(list(params_std.values()), dtype=float) + 1e-3 * rng.standard_normal(len(W_ref))
    outs = {}
    for rule in (True, False):
        pipe = IdentificationPipeline(robot, param, params_std=params_std, null_pivots=rule)
        pipe.set_samples(q, v, a, tau)
        outs[rule] = pipe.run()
        outs[rule] = pipe.run()
        if rule:
            fell_back = pipe.null_rule_fallbacks
    assert outs[True]["idx_e"] == outs[False]["idx_e"] and outs[True]["idx_base"] == outs[False]["idx_base"]
    assert abs(outs[True]["residual_norm"] - outs[False]["residual_norm"]) <= 1e-9 * max(1.0, outs[False]["residual_norm"])
    # LAPACK on the oracle's matrix: the same classification (pivots of an unpivoted QR of a rank-deficient matrix: decision only)
    kept = [i for i in range(W_ref.shape[1]) if i not in set(outs[False]["idx_e"])]
    d_ref = np.abs(np.diag(np.linalg.qr(W_ref[:, kept], mode="r")))
    lap = [i for i in range(len(kept)) if d_ref[i] > TOL_QR]
    if min(np.abs(d_ref - TOL_QR)) > 0.5 * TOL_QR:  # (LAPACK's own near-tolerance pivots are not comparable across orders)
        assert lap == outs[False]["idx_base"]
    # the drop-in mirror certifies as well
    params_r = outs[False]["params_r"]
    assert list(get_baseIndex(np.ascontiguousarray(W_ref[:, kept]), params_r)) == \
        list(get_baseIndex(np.ascontiguousarray(W_ref[:, kept]), params_r, null_pivots=False)) == outs[False]["idx_base"]
    assert fell_back >= 0  # (whether THIS sample set trips the certificate depends on the samples; the result may not)


@pytest.mark.parametrize("seed", range(16))
def test_tree_walks_fuzz(lib, oracle_lib, seed):
    """Random trees (8 .. 30 joints, random depth / branching, random joint types, some massless links) through both walks of
    the tape kernel against the C oracle: the joint-torque regressor in the reference's dense layout, and -- with a free-flyer
    root on top of the same tree -- the external-wrench regressor through the pipeline's default (force-compact, state copy at
    branch joints) and link-padded layouts (column norms against the oracle, identical index sets)."""
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from figaroh_plus_amd.tools.regressor import build_regressor_basic
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(8, 31))
    parents = _random_parents(rng, n, deep=float(rng.choice([0.4, 0.6, 0.8])))
    massless = tuple(int(k) for k in rng.choice(np.arange(2, n + 1), size=n // 6, replace=False))
    N = 64 * 2 + int(rng.integers(1, 64))

    def inputs(m, free):
        q = np.zeros((N, m.nq))
        for j in m.joints[1:]:
            if j.nq == 7:
                quat = rng.standard_normal((N, 4))
                q[:, :3], q[:, 3:7] = rng.uniform(-1, 1, (N, 3)), quat / np.linalg.norm(quat, axis=1)[:, None]
            elif j.nq == 2:
                th = rng.uniform(-3, 3, N)
                q[:, j.idx_q], q[:, j.idx_q + 1] = np.cos(th), np.sin(th)
            else:
                q[:, j.idx_q] = rng.uniform(-2, 2, N)
        return q, rng.uniform(-2, 2, (N, m.nv)), rng.uniform(-3, 3, (N, m.nv))

    # joint torques, fixed base
    robot = _synthetic_tree(parents, seed=seed, massless=massless)
    param = dict(is_joint_torques=True, is_external_wrench=False, has_friction=bool(seed & 1), has_actuator_inertia=bool(seed & 2),
                 has_joint_offset=bool(seed & 4), force_torque=None)
    q, v, a = inputs(robot.model, False)
    mode, fl, ft = oracle_lib.param_flags(param, False)
    W_ref = oracle_lib.OracleModel(robot.model.to_flat()).build_regressor_basic(q, v, a, mode, fl, ft)
    W = build_regressor_basic(robot, q, v, a, param)
    assert np.abs(W - W_ref).max() <= 1e-12 * np.abs(W_ref).max(), parents
    # external wrench, the same tree under a free-flyer root
    if n > 25:
        return  # (the wrench models stay below the 32 links of the pipeline's layouts comfortably)
    robot = _synthetic_tree([0] + [p + 1 for p in parents], seed=seed, massless=tuple(k + 1 for k in massless), freeflyer=True)
    m = robot.model
    param = dict(is_joint_torques=False, is_external_wrench=True, has_friction=False, has_actuator_inertia=False,
                 has_joint_offset=False, force_torque=["All"])
    N = 64 * 90 + int(rng.integers(1, 64))  # (the force / torque split wants 32 rows per kept column)
    q, v, a = inputs(m, True)
    mode, fl, ft = oracle_lib.param_flags(param, False)
    W_ref = oracle_lib.OracleModel(m.to_flat()).build_regressor_basic(q, v, a, mode, fl, ft)
    ref_sq = (W_ref * W_ref).sum(axis=0)
    params_std = robot.get_standard_parameters(param)
    tau = W_ref @ np.array(list(params_std.values()), dtype=float) + 1e-3 * rng.standard_normal(len(W_ref))
    outs = []
    for layout in ("link-padded", "dense"):
        pipe = IdentificationPipeline(robot, param, params_std=params_std, w_layout=layout)
        pipe.set_samples(q, v, a, tau)
        pipe.run()
        outs.append(pipe.run())
        assert np.abs(outs[-1]["col_norm"] - ref_sq).max() <= 1e-12 * ref_sq.max(), (layout, parents)
    assert outs[0]["idx_e"] == outs[1]["idx_e"] and outs[0]["idx_base"] == outs[1]["idx_base"]
    # (the two layouts sum in different orders: on a base regressor whose extreme pivots are a factor 1e11 apart -- random inertias;
    # fuzz seeds 3027, 3428: a base pivot of 1.5e-8 -- the residual is only determined to cond eps; LAPACK's lstsq and its QR differ
    # by 1e-5 relative there)
    bp = outs[0]["absdiagR"][np.asarray(outs[0]["idx_base"])]
    res_tol = max(1e-9, 10 * np.finfo(float).eps * bp.max() / bp.min())
    assert abs(outs[0]["residual_norm"] - outs[1]["residual_norm"]) <= res_tol * max(1.0, outs[0]["residual_norm"]), (
        outs[0]["residual_norm"], outs[1]["residual_norm"], float(np.linalg.norm(tau)), parents)
    # (round 6) ... and the classification is LAPACK's on the oracle's matrix, wherever LAPACK's own pivots keep clear of the
    # tolerances (random inertias make ill-conditioned models: this is what found the spurious base parameters of the unguarded
    # null-pivot rule, tools/fuzz_trees.py)
    idx_e = [int(i) for i in range(W_ref.shape[1]) if ref_sq[i] < 1e-6]
    kept = [i for i in range(W_ref.shape[1]) if not ref_sq[i] < 1e-6]
    d_ref = np.abs(np.diag(np.linalg.qr(W_ref[:, kept], mode="r")))
    if np.abs(d_ref - 1e-8).min() > 0.5e-8 and np.abs(ref_sq - 1e-6).min() > 0.5e-6:
        assert outs[0]["idx_e"] == idx_e
        assert outs[0]["idx_base"] == [i for i in range(len(kept)) if d_ref[i] > 1e-8], parents
