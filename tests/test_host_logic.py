"""CPU suite, part 3: host-side glue of the drop-in API (no kernels involved)."""
import io
import contextlib
import os

import numpy as np
import pytest

import oracle_np
from conftest import ROOT


def test_standard_parameter_names_and_values(golden):
    robot = golden.robot()
    with contextlib.redirect_stdout(io.StringIO()):
        std = robot.get_standard_parameters(golden.param)
    names = golden.meta["names_std"][:len(std)]
    assert list(std.keys()) == names
    ref = golden.meta["phi_ref_raw"][:len(std)]
    assert [float(x) for x in std.values()] == [float(x) for x in ref]
    assert list(std.values())[10] == ref[10]  # YAML strings stay strings (T40X_config.yaml:17-20 quirk)


def test_model_attributes_mirror_pinocchio(golden):
    robot = golden.robot()
    m = robot.model
    d = golden.meta["dims"]
    assert (m.njoints, m.nq, m.nv) == (d["njoints"], d["nq"], d["nv"])
    assert m.names == golden.meta["joint_names"]
    assert [j for j in range(len(m.inertias.tolist())) if m.inertias.tolist()[j].mass != 0] == golden.meta["id_inertias"]
    assert m.joints[m.njoints - 1].idx_v + m.joints[m.njoints - 1].nv == m.nv
    assert robot.q0.shape == (m.nq,) and robot.v0.shape == (m.nv,)
    assert m.getJointId(m.names[2]) == 2 and m.getJointId("nope") == m.njoints


def test_flat_roundtrip(golden, tmp_path):
    from figaroh_plus_amd.model import Model
    m = golden.robot().model
    p = tmp_path / "m.json"
    m.save_flat(str(p))
    f1, f2 = m.to_flat(), Model.from_flat(str(p)).to_flat()
    for k in ("parents", "jtype", "idx_q", "idx_v", "axis", "placement", "mass", "lever", "inertia"):
        assert np.array_equal(np.asarray(f1[k]), np.asarray(f2[k])), k


def test_expression_strings_match_reference_format(golden):
    from figaroh_plus_amd.tools import qrdecomposition as qrd
    g = golden
    W = oracle_np.build_regressor_basic(g.flat(), g["q_big"], g["v_big"], g["a_big"], g.param)
    if g.coupling:
        W = oracle_np.add_coupling_TX40(W, len(g["q_big"]), g["v_big"], g["a_big"])
    W_e = np.delete(W, g["idx_e"], 1)
    params_r = g.meta["params_r"]
    res = oracle_np.base_parameters(W_e, params_r)
    idx_base = res["idx_base"]
    idx_regroup = [i for i in range(len(params_r)) if i not in set(idx_base)]
    got = qrd._expressions([params_r[i] for i in idx_base], [params_r[i] for i in idx_regroup], res["beta"])
    assert got == g.meta["params_base"]
    ib, ir = qrd._select(res["diagR"], params_r, 1e-8)
    assert ib == list(g["idx_base"]) and ir == idx_regroup
    with pytest.raises(AssertionError):
        qrd._select(res["diagR"], params_r[:-1], 1e-8)


def test_base_param_from_standard_and_index(golden):
    from figaroh_plus_amd.identification.identification_tools import base_param_from_standard, index_in_base_params
    g = golden
    std = {k: float(v) for k, v in g.params_std().items()}
    vals = np.array(base_param_from_standard(std, g.meta["params_base"]), dtype=float)
    assert np.allclose(vals, g["phi_from_std"], rtol=0, atol=1e-12)
    segs = [1, 2]
    idx = index_in_base_params(g.meta["params_base"], segs)
    for k, seg in enumerate(segs):
        if k in idx:
            for ii in idx[k]:
                assert any(tok.split("*")[-1][-len(str(seg)):] == str(seg) for tok in g.meta["params_base"][ii].split(" "))


def test_param_from_yaml_keys(golden_ur10):
    from figaroh_plus_amd.identification.identification_tools import get_param_from_yaml
    import yaml
    cfg = {"robot_params": [{"q_lim_def": 1.57, "dq_lim_def": 5.0, "fv": None, "fs": None, "Ia": None, "offset": None,
                             "Iam6": None, "fvm6": None, "fsm6": None, "N": None, "ratio_essential": None}],
           "problem_params": [{"is_external_wrench": False, "is_joint_torques": True, "force_torque": ["All"],
                               "external_wrench_offsets": False, "has_friction": False, "has_joint_offset": False,
                               "has_actuator_inertia": False, "has_coupled_wrist": False}],
           "processing_params": [{"cut_off_frequency_butterworth": 100.0, "ts": 0.01}],
           "tls_params": [{"mass_load": None, "which_body_loaded": None}]}
    cfg = yaml.safe_load(yaml.safe_dump(cfg))
    param = get_param_from_yaml(golden_ur10.robot(), cfg)
    ref = golden_ur10.param
    assert set(param) == set(ref)
    assert param["nb_samples"] == ref["nb_samples"] == 100
    for k in ("is_joint_torques", "has_friction", "force_torque", "ts"):
        assert param[k] == ref[k]


def test_regressor_flags_and_errors(golden):
    from figaroh_plus_amd import _lib
    from figaroh_plus_amd.tools.regressor import regressor_flags
    mode, flags, ft = regressor_flags(golden.param, golden.coupling)
    assert mode == (0 if golden.param["is_joint_torques"] else 1)
    assert bool(flags & _lib.FLAG_FRICTION) == bool(golden.param["has_friction"])
    assert bool(flags & _lib.FLAG_TX40) == golden.coupling
    bad = dict(golden.param, is_joint_torques=False, is_external_wrench=True, force_torque=["Fx", "bogus"])
    with pytest.raises(ValueError, match="Please enter valid parameters"):
        regressor_flags(bad)
    ok = dict(bad, force_torque=["Fx", "Mz"])
    assert regressor_flags(ok)[2] == (1 | 32)
    neither = dict(golden.param, is_joint_torques=False, is_external_wrench=False)
    with pytest.raises(UnboundLocalError):
        regressor_flags(neither)


def test_pipeline_rejects_mismatched_sample_shapes(golden_ur10):
    """IdentificationPipeline.set_samples must validate shapes before anything is uploaded (a wrong v / a /
    tau would be read past its HBM allocation by K1 / K3).  No device is needed: the checks run first."""
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    g = golden_ur10
    pipe = IdentificationPipeline(g.robot(), g.param, params_std=g.params_std())
    q, v, a = g["q_big"], g["v_big"], g["a_big"]
    N = len(q)
    with pytest.raises(ValueError):
        pipe.set_samples(q, v[:, :5], a)                 # v with nv - 1 columns
    with pytest.raises(ValueError):
        pipe.set_samples(q, v, a[:N - 1])                # a with a row missing
    with pytest.raises(ValueError):
        pipe.set_samples(q, v, a, tau=np.zeros(6 * N + 1))  # tau from another run


def test_free_flyer_differentiation_matches_reference():
    """calculate_first_second_order_differentiation on the human model (free-flyer root: pin.difference = SE(3) log),
    constant and variable time steps, against the output of the reference's own function (oracle/gen_golden_extra.py;
    VERDICT r01: the mirror used to raise NotImplementedError here).  Host NumPy: no device needed."""
    from figaroh_plus_amd.identification.identification_tools import (calculate_first_second_order_differentiation,
                                                                       joint_difference)
    from figaroh_plus_amd.tools.robot import Robot
    z = np.load(os.path.join(ROOT, "tests", "golden", "human_differentiation.npz"))
    model = Robot.from_flat("human").model
    param = {"is_joint_torques": False, "is_external_wrench": True, "ts": float(z["ts"])}
    q, dq, ddq = calculate_first_second_order_differentiation(model, z["q"], param)
    assert np.array_equal(q, z["q_out"])
    assert np.abs(dq - z["dq"]).max() <= 1e-12 * np.abs(z["dq"]).max()
    assert np.abs(ddq - z["ddq"]).max() <= 1e-12 * np.abs(z["ddq"]).max()
    q, dq, ddq = calculate_first_second_order_differentiation(model, z["q"], param, dt=z["dt"])
    assert np.abs(dq - z["dq_dt"]).max() <= 1e-12 * np.abs(z["dq_dt"]).max()
    assert np.abs(ddq - z["ddq_dt"]).max() <= 1e-12 * np.abs(z["ddq_dt"]).max()
    # the free-flyer block is a genuine SE(3) difference, not q1 - q0
    d = joint_difference(model, z["q"][0], z["q"][1])
    assert np.abs(d[:3] - (z["q"][1, :3] - z["q"][0, :3])).max() > 1e-6
    assert np.abs(oracle_np.joint_difference(model.to_flat(), z["q"][0], z["q"][1]) - d).max() <= 1e-14


# ------------------------------------------------------------------------------------------------ 8f-3 SIP program
def _sip_fixture(cfg):
    z = np.load(os.path.join(ROOT, "tests", "golden", "sip_qp.npz"))
    g = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(cfg + "/")}
    C = np.zeros((len(g["qp_a"]), len(g["qp_b"])))
    C[g["qp_C_row"], np.arange(len(g["qp_b"]))] = g["qp_C_val"]
    g["qp_C"] = C
    return g


def _kkt(G, a, C, b, meq, x, lag):
    s = C.T @ x - b
    return {"stationarity": np.abs(G @ x - a - C @ lag).max(),
            "primal": max(0.0, -s[meq:].min() if len(s) > meq else 0.0, np.abs(s[:meq]).max() if meq else 0.0),
            "dual": max(0.0, -lag[meq:].min()) if len(lag) > meq else 0.0,
            "complementarity": np.abs(lag[meq:] * s[meq:]).max() if len(s) > meq else 0.0}


def test_qp_solver_satisfies_kkt_on_random_programs():
    """The host Goldfarb-Idnani solver (identification/qp.py, the reference's quadprog.solve_qp): for a strictly
    convex program the KKT conditions are necessary and sufficient, so they pin the solution; equality rows, dependent
    and never-active constraints, drops from the active set included."""
    from figaroh_plus_amd.identification.qp import solve_qp
    rng = np.random.default_rng(11)
    removed = 0
    for trial in range(40):
        n = int(rng.integers(2, 40))
        m = int(rng.integers(0, 60))
        meq = int(rng.integers(0, min(n, m) // 2 + 1)) if m else 0
        A = rng.standard_normal((n + 5, n))
        G = A.T @ A + 0.1 * np.eye(n)
        a = 3 * rng.standard_normal(n)
        C = rng.standard_normal((n, m))
        x0 = rng.standard_normal(n)
        b = C.T @ x0 - rng.uniform(0, 1, m)
        b[:meq] = C[:, :meq].T @ x0
        x, f, xu, it, lag, iact = solve_qp(G, a, C, b, meq)
        assert max(_kkt(G, a, C, b, meq, x, lag).values()) <= 1e-9, trial
        assert abs(f - (0.5 * x @ G @ x - a @ x)) <= 1e-9 * (1 + abs(f))
        assert np.abs(G @ xu - a).max() <= 1e-9 * np.abs(a).max()
        assert sorted(iact.tolist()) == sorted((np.flatnonzero(lag != 0) + 1).tolist()) or len(iact) >= (lag != 0).sum()
        removed += int(it[1])
    assert removed > 0  # the sweep exercised the partial-step / drop branch
    # quadprog's error behaviour
    with pytest.raises(ValueError, match="positive definite"):
        solve_qp(-np.eye(2), np.zeros(2))
    with pytest.raises(ValueError, match="inconsistent"):
        solve_qp(np.eye(2), np.zeros(2), np.array([[1.0, -1.0], [0.0, 0.0]]), np.array([1.0, 1.0]))  # x0 >= 1, x0 <= -1
    x = solve_qp(np.eye(3), np.array([1.0, 2.0, 3.0]))[0]  # no constraints: the unconstrained minimiser
    assert np.allclose(x, [1, 2, 3])


@pytest.mark.parametrize("cfg", ["cfg4_talos", "cfg5_human"])
def test_sip_program_against_reference_fixture(cfg):
    """The SIP program of calculate_standard_parameters (identification_tools.py:466-572): tests/golden/sip_qp.npz holds
    what the reference's own function hands to quadprog.solve_qp (recorded by oracle/gen_golden_extra.py) and the
    solution of that program from an independent bounded-least-squares solve.  Host side of the mirror: the bound rows
    G, h, quadprog_solve_qp's regularisation / sign conventions, and the solver."""
    from figaroh_plus_amd.identification.identification_tools import quadprog_solve_qp, sip_constraints
    from figaroh_plus_amd.identification.qp import solve_qp
    g = _sip_fixture(cfg)
    G, h = sip_constraints(g["phi_ref"], g["COM_max"], g["COM_min"])
    assert np.array_equal(-G.T, g["qp_C"]) and np.array_equal(-h, g["qp_b"]) and int(g["meq"]) == 0
    x, f, xu, it, lag, iact = solve_qp(g["qp_G"], g["qp_a"], g["qp_C"], g["qp_b"], 0)
    scale = np.abs(g["phi_standard"]).max()
    assert np.abs(x - g["phi_standard"]).max() <= 1e-10 * scale
    assert max(_kkt(g["qp_G"], g["qp_a"], g["qp_C"], g["qp_b"], 0, x, lag).values()) <= 1e-12
    # through the reference's wrapper: P, q with G x <= h (qp_G = 0.5 (P + P^T) + 1e-5 I, qp_a = -q)
    n = len(x)
    P = g["qp_G"] - 1e-5 * np.eye(n)
    x2 = quadprog_solve_qp(P, -g["qp_a"], G, h)
    assert np.abs(x2 - g["phi_standard"]).max() <= 1e-10 * scale
    # an equality row through the wrapper (A x = b): total mass fixed to the reference's
    A = np.zeros((1, n))
    A[0, 9::10] = 1.0
    bm = np.array([g["phi_ref"][9::10].sum()])
    x3 = quadprog_solve_qp(P, -g["qp_a"], G, h, A, bm)
    assert abs(x3[9::10].sum() - bm[0]) <= 1e-10 * bm[0] and (G @ x3 <= h + 1e-10 * scale).all()


def test_calibration_parameter_names():
    """get_geo_offset / get_joint_offset (calibration_tools.py:252-331): six placement offsets per joint, one joint
    offset per degree of freedom named after Pinocchio's joint model (axis-aligned: RZ, PX, RUBZ ...; multi-dof joints
    number their entries from the second one)."""
    from figaroh_plus_amd.calibration.calibration_tools import get_geo_offset, get_joint_offset
    from figaroh_plus_amd.tools.robot import Robot
    m = Robot.from_flat("tx40").model
    geo = get_geo_offset(list(m.names[1:]))
    assert list(geo)[:7] == ["d_px_joint_1", "d_py_joint_1", "d_pz_joint_1", "d_phix_joint_1", "d_phiy_joint_1",
                             "d_phiz_joint_1", "d_px_joint_2"] and set(geo.values()) == {0}
    assert list(get_joint_offset(m, m.names[1:])) == ["offsetRZ_joint_%d" % k for k in range(1, 7)]
    t = Robot.from_flat("talos").model
    off = list(get_joint_offset(t, t.names[1:]))
    assert off[:7] == ["offsetFreeFlyer_root_joint"] + ["offsetFreeFlyer%d_root_joint" % k for k in range(2, 7)] + \
        ["offsetRZ_leg_left_1_joint"] and len(off) == t.nv
    # the fixture's names were produced by the reference's own get_geo_offset / get_joint_offset
    import json
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "calibration_base_regressor.json")))
    assert set(ref["tx40_full"]["paramsrand_e"]) <= set(geo)
    assert set(ref["talos_offsets"]["paramsrand_e"]) <= set(off)


def test_set_missing_params_setting_matches_reference():
    """identification_tools.py:86-165 against what the reference's own function returns, prints and does to the model
    (tests/golden/missing_params.json, oracle/gen_golden_missing_params.py)."""
    import contextlib
    import io
    import json
    import os
    import types
    from figaroh_plus_amd.identification.identification_tools import set_missing_params_setting
    with open(os.path.join(os.path.dirname(__file__), "golden", "missing_params.json")) as f:
        fixtures = json.load(f)
    for name, fx in fixtures.items():
        c = fx["input"]
        model = types.SimpleNamespace(lowerPositionLimit=np.array(c["lower"]), upperPositionLimit=np.array(c["upper"]),
                                      velocityLimit=np.array(c["velocity"]), effortLimit=np.array(c["effort"]),
                                      nq=c["nq"], nv=c["nv"])
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res = set_missing_params_setting(types.SimpleNamespace(model=model), dict(c["settings"]))
        assert buf.getvalue() == fx["printed"], name
        got = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in res.items()}
        assert got == fx["result"], name
        after = fx["model_after"]
        assert model.lowerPositionLimit.tolist() == after["lower"] and model.upperPositionLimit.tolist() == after["upper"]
        assert model.velocityLimit.tolist() == after["velocity"] and model.effortLimit.tolist() == after["effort"]


def test_essential_parameters_from_triangles_equals_script_loop():
    """identification_tools.essential_parameters (the loop of examples/staubli_TX40/identification.py:354-399 run on the two
    small triangles of a pass) against the oracle's statement-for-statement loop on the full W_b: same parameters dropped in
    the same order, same rounded estimates.  Host only: the triangles come from LAPACK here."""
    import oracle_np
    from figaroh_plus_amd.identification.identification_tools import essential_parameters
    rng = np.random.default_rng(12)
    counts = [400, 380, 410, 395]
    m, r = sum(counts), 9
    W_b = rng.standard_normal((m, r)) * np.array([1, 1, 1, 1, 0.05, 1, 0.02, 1, 0.01])  # three poorly excited parameters
    phi_true = rng.uniform(0.5, 2.0, r)
    noise = np.repeat([0.05, 0.1, 0.2, 0.07], counts)
    tau = W_b @ phi_true + noise * rng.standard_normal(m)
    names = ["p%d" % i for i in range(r)]
    phi_b = np.around(np.linalg.lstsq(W_b, tau, rcond=None)[0], 6)
    sig2, a = [], 0
    for n in counts:
        sig2.append(np.linalg.norm(tau[a:a + n] - W_b[a:a + n] @ phi_b) ** 2 / n)
        a += n
    phi_w, std_w = oracle_np.wls_script(W_b, tau, phi_b, counts)
    ref = oracle_np.essential_script(W_b, tau, names, std_w, sig2, counts, 30.0)
    assert ref["iterations"] >= 2
    sw = np.repeat(1.0 / np.sqrt(sig2), counts)
    R_ols = np.linalg.qr(np.c_[W_b, tau], mode="r")
    R_wls = np.linalg.qr(np.c_[W_b * sw[:, None], tau * sw], mode="r")
    got = essential_parameters(R_ols, R_wls, names, std_w, 30.0, rows_total=m)
    assert got["params_essential"] == ref["params_essential"] and got["iterations"] == ref["iterations"]
    assert np.abs(got["phi_e_ols"] - ref["phi_e_ols"]).max() <= 1.5e-6
    assert np.abs(got["phi_e_wls"] - ref["phi_e_wls"]).max() <= 1.5e-6
    assert np.abs(got["std_e_wls"] - ref["std_e_wls"]).max() <= 0.011
    assert np.abs(got["std_e_ols"] - ref["std_e_ols"]).max() <= 0.011
    # a tie for the largest std%: the script's int(i) raises; so does the mirror, instead of dropping the first silently
    tied = np.array(std_w, dtype=float)
    tied[[2, 5]] = tied.max() + 50.0
    with pytest.raises(TypeError, match="length-1"):
        essential_parameters(R_ols, R_wls, names, tied, 30.0, rows_total=m)


def test_relative_percent_zero_estimate_is_inf_without_warning():
    """std% of an estimate that rounds to exactly zero: the reference's 100 sqrt(C_ii) / |phi_i| is inf (NumPy division by
    zero, identification_tools.py:226-232); the mirrors return the same inf deliberately, without the RuntimeWarning."""
    import warnings
    from figaroh_plus_amd._host import relative_percent
    sigma, phi = np.array([0.5, 0.25, 0.0, 2.0]), np.array([2.0, 0.0, 0.0, -4.0])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = relative_percent(sigma, phi)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.round(100 * sigma / np.abs(phi), 2)
    assert np.array_equal(got, want, equal_nan=True) and np.isinf(got[1]) and np.isnan(got[2])


def test_null_rule_certificate():
    """_host.null_rule_bounds / null_rule_certified (round 6): the a-posteriori certificate of the null-pivot rule.  The
    coefficient sums are those of the regrouped triangle; a classification is certified only when every pivot is further from
    tol_qr than (1 + A) x the folded tol_qr / 64 (x 2)."""
    from figaroh_plus_amd._host import null_rule_bounds, null_rule_certified
    tol = 1e-8
    R1 = np.array([[1.0, 2.0, -3.0], [0.0, 1e-3, 4e-3], [0.0, 0.0, 5.0]])
    R2 = np.c_[R1 @ np.ones(3), np.zeros(3)]  # first dependent column = 1 b0 + 1 b1 + 1 b2, second = 0
    A_base, A_dep, xnorm = null_rule_bounds(R1, R2)
    assert xnorm == pytest.approx(np.abs(np.linalg.inv(R1)).sum(axis=1).max())
    # A_base[k] = sum |R1[:k,:k]^-1 R1[:k,k]|
    want = [0.0, 2.0, np.abs(np.linalg.solve(R1[:2, :2], R1[:2, 2])).sum()]
    assert np.allclose(A_base, want, rtol=1e-12)
    assert np.allclose(A_dep, [3.0, 0.0], rtol=1e-12)
    diag = np.array([1.0, 1e-3, 5.0, 1e-12, 0.0])
    assert null_rule_certified(diag, [0, 1, 2], [3, 4], (A_base, A_dep, xnorm), tol)
    # a base pivot 2 % above the tolerance with A = 2: margin 2e-10 < 2 (1 + 2) 1.5625e-10 -> not certified
    assert not null_rule_certified(np.array([1.0, 1.02e-8, 5.0, 1e-12, 0.0]), [0, 1, 2], [3, 4], (A_base, A_dep, xnorm), tol)
    # ... 20 % above it is
    assert null_rule_certified(np.array([1.0, 1.2e-8, 5.0, 1e-12, 0.0]), [0, 1, 2], [3, 4], (A_base, A_dep, xnorm), tol)
    # a dependent pivot just below the tolerance is not
    assert not null_rule_certified(np.array([1.0, 1e-3, 5.0, 0.95e-8, 0.0]), [0, 1, 2], [3, 4], (A_base, A_dep, xnorm), tol)
    # a dependent column with genuine content of its own (above tol / 8) may have been folded entirely: not certified
    assert not null_rule_certified(np.array([1.0, 1e-3, 5.0, 2e-9, 0.0]), [0, 1, 2], [3, 4], (A_base, A_dep, xnorm), tol)
    assert null_rule_certified(np.array([1.0, 1e-3, 5.0, 1.5e-10, 1e-13]), [0, 1, 2], [3, 4], (A_base, A_dep, xnorm), tol)
    # large regrouping coefficients: the folded 1.6e-10 could surface as a pivot above the tolerance
    assert not null_rule_certified(diag, [0, 1, 2], [3, 4], (A_base, np.array([700.0, 0.0]), xnorm), tol)
    # a spurious base column shows as a tiny R1_kk with huge projection coefficients
    R1s = np.array([[1.0, 500.0], [0.0, 1.1e-7]])
    Ab, Ad, xn = null_rule_bounds(R1s, np.zeros((2, 0)))
    assert Ab[1] == pytest.approx(500.0) and not null_rule_certified(np.array([1.0, 1.1e-7]), [0, 1], [], (Ab, Ad, xn), tol)
    # the estimates themselves: |R1^-1|_inf (tol / 64) |phi|_1 against 1e-7 |phi|_inf
    assert null_rule_certified(diag, [0, 1, 2], [3, 4], (A_base, A_dep, 1.0), tol, phi=np.array([3.0, -2.0, 1.0]))
    assert not null_rule_certified(diag, [0, 1, 2], [3, 4], (A_base, A_dep, 1e4), tol, phi=np.array([3.0, -2.0, 1.0]))
    assert null_rule_bounds(np.array([[1.0, 1.0], [0.0, 0.0]]), np.zeros((2, 0))) is None  # singular: never certified
    assert not null_rule_certified(diag, [0, 1, 2], [3, 4], None, tol)


def test_bench_spawns_rank_processes_and_relays_their_failure():
    """`python bench.py --gpus 2` with no launcher (WORLD_SIZE unset) starts two rank processes itself (bench.spawn_ranks) and exits
    with a child's non-zero code when they fail -- here because this container has no HIP device and the product has no CPU path
    (the GPU box runs the same command to completion: test_bench_spawns_its_own_ranks)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")
           and not k.startswith("FIGH_")}
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    if "needs a HIP device" in out:  # (the CPU container; on a GPU box the ranks run, which the GPU suite checks)
        assert p.returncode != 0 and out.count("needs a HIP device") == 2, out[-2000:]
    else:
        # one line, rank 0's (it quotes n_gpus for the headline and again for strong_scaling)
        lines = [json.loads(line) for line in out.splitlines() if line.startswith("{")]
        assert p.returncode == 0 and len(lines) == 1 and lines[0]["n_gpus"] == 2, out[-2000:]


def test_null_rule_certificate_sqrt_triangles():
    """With the rows of the factorisation, a base pivot must clear tol_qr by 2 (1 + A) sqrt(T) tol_qr / 64: a genuine base
    column folded in almost every level-0 triangle leaks up to sqrt(T) tol_qr / 64 into the columns behind it (the
    adversarial family of test_qr_graded.py: 4e6 rows, a spurious pivot above tol_qr).  Large pivots stay certified."""
    from figaroh_plus_amd._host import null_rule_bounds, null_rule_certified, null_rule_triangles
    tol = 1e-8
    R1 = np.array([[1.0, 2.0, -3.0], [0.0, 4.5e-8, 4e-3], [0.0, 0.0, 5.0]])
    bounds = null_rule_bounds(R1, np.c_[R1 @ np.ones(3), np.zeros(3)])
    diag = np.array([1.0, 4.5e-8, 5.0, 1e-12, 0.0])
    assert null_rule_triangles(4000000) == 125001 and null_rule_triangles(1) == 2 and null_rule_triangles(64, 24) == 26
    assert null_rule_certified(diag, [0, 1, 2], [3, 4], bounds, tol)  # the per-triangle margin alone lets it through
    assert null_rule_certified(diag, [0, 1, 2], [3, 4], bounds, tol, rows=64)
    assert not null_rule_certified(diag, [0, 1, 2], [3, 4], bounds, tol, rows=4000000)
    big = np.array([1.0, 4e3, 5.0, 1e-12, 0.0])  # UR10 / TALOS / human: smallest base pivots 4e3 .. 6e3 at full size
    R1b = R1.copy()
    R1b[1, 1] = 4e3
    assert null_rule_certified(big, [0, 1, 2], [3, 4], null_rule_bounds(R1b, np.c_[R1b @ np.ones(3), np.zeros(3)]), tol,
                               rows=6 * 10 ** 7)


def test_graded_qr_exact_gram_against_python_integers():
    """tests/qr_graded_common.exact_gram: the Gram of an integer matrix with power-of-two column scales and row block
    weights equals Python-integer (exact rational) arithmetic."""
    from fractions import Fraction

    import qr_graded_common as qg
    rng = np.random.default_rng(3)
    M = qg.int_matrix(rng, 37, 6)
    s = np.array([-30, 7, 0, -10, 30, 3])
    e = np.repeat([-1, 0, 1], [10, 20, 7])
    G = qg.exact_gram(M, s, e)
    for i in range(6):
        for j in range(6):
            want = sum(Fraction(int(M[r, i]) * int(M[r, j])) * Fraction(2) ** int(2 * e[r]) for r in range(37))
            want *= Fraction(2) ** int(s[i] + s[j])
            assert Fraction(G[i, j]) == want
    with pytest.raises(AssertionError):
        qg.exact_gram(M + 0.5, s)


@pytest.mark.parametrize("n", [1, 7, 40])
def test_graded_qr_longdouble_cholesky_against_mpmath(n):
    """tests/qr_graded_common.cholesky_ld against a 50-digit mpmath Cholesky of the same exact Gram, column by column."""
    mpmath = pytest.importorskip("mpmath")
    import qr_graded_common as qg
    rng = np.random.default_rng(n)
    M = qg.int_matrix(rng, 3 * n + 5, n)
    s = qg.graded_scales(rng, n, -30, 30, [0, n - 1])
    G = qg.exact_gram(M, s)
    R = qg.cholesky_ld(G)
    mpmath.mp.dps = 50
    Rm = mpmath.cholesky(mpmath.matrix([[mpmath.mpf(float(x)) for x in row] for row in G])).T
    nrm = qg.col_norms(G)
    cond = qg.equilibrated_cond(R)
    for j in range(n):
        col = [mpmath.mpf(a) / b for a, b in (R[i, j].as_integer_ratio() for i in range(n))]  # (exact: 64-bit mantissas)
        err = mpmath.sqrt(sum((col[i] - Rm[i, j]) ** 2 for i in range(n)))
        assert float(err) / nrm[j] <= 64 * cond * cond * 2.0 ** -64


def test_graded_qr_columnwise_metric_rejects_what_the_normwise_check_accepts():
    """A planted error: LAPACK's R with a 1e-9 relative error in a 2^-20-scaled column.  The suite's older norm-wise check
    (|R^T R - G| <= 1e-12 max |G|) accepts it; the column-wise metrics of test_qr_graded.py reject it."""
    import qr_graded_common as qg
    rng = np.random.default_rng(20)
    n, rows = 30, 400
    M = qg.int_matrix(rng, rows, n)
    s = np.zeros(n, dtype=np.int64)
    s[11] = -20
    G = qg.exact_gram(M, s)
    R = np.linalg.qr(M * np.ldexp(1.0, s), mode="r")
    R_ref = qg.cholesky_ld(G)
    cond = qg.equilibrated_cond(R_ref)
    assert qg.backward_err(R, G) <= 1e-13 and qg.forward_err(R, R_ref, G) <= 200 * cond * 2.0 ** -53  # clean: both pass
    R[:, 11] *= 1.0 + 1e-9
    assert qg.normwise_backward_err(R, G) <= 1e-12
    assert qg.backward_err(R, G) > 1e-13
    assert qg.forward_err(R, R_ref, G) > 200 * cond * 2.0 ** -53
    assert qg.diag_err(R, R_ref, G) > 200 * cond * 2.0 ** -53


# ------------------------------------------------------------------ structured graded generators (test_qr_structured_graded.py)
@pytest.mark.parametrize("extra,dead_links,deps", [(True, (), False), (True, (2,), True), (False, (1, 4), True)])
def test_wrench_generator_structure_layouts_and_gram(extra, dead_links, deps):
    """tests/qr_graded_common.Wrench: the Gram is exact, the force rows are zero on slots < 6, the dependencies are exact
    (and keep that zero pattern), and every device layout reads back to the reference-layout W."""
    import qr_graded_common as qg
    rng = np.random.default_rng([7, len(dead_links), int(deps)])
    g = qg.Wrench(rng, 37, 6, 40 if extra else 36, -30, 30, dead_links=dead_links, extra_slots=extra, deps=deps)
    W = g.reference()
    assert not W[:3 * g.Nb][:, (np.arange(g.ncols) % 14) < 6].any()
    assert np.count_nonzero(np.any(W != 0, axis=0)) == g.n and g.n <= 0.8 * g.ncols
    if not extra:
        assert not W[:, (np.arange(g.ncols) % 14) >= 10].any()
    G = g.gram()
    A = np.c_[W[:, g.kept], g.tau()]
    assert np.array_equal(G, np.asarray(np.asarray(A, dtype=np.longdouble).T @ np.asarray(A, dtype=np.longdouble),
                                        dtype=np.float64))
    for k in g.dep:  # an inertia column stays zero in the force rows
        assert g.slot[k] >= 6 or not W[:3 * g.Nb, g.kept[k]].any()
    if deps:
        assert len(g.dep) > 5
        Gb = qg.cholesky_ld(g.gram(False)[np.ix_(g.base, g.base)])
        assert float(np.diag(Gb).min()) > 0
        R = np.linalg.qr(g.A(), mode="r")
        assert (np.abs(np.diag(R))[g.dep] < 1e-6 * np.abs(np.diag(R)).max()).all()
    # the layouts as figh.h states them, entry by entry (independent of the column maps the writers and readers share)
    Wp, Wc = g.padded(), g.padded(compact=True)
    for c in range(g.ncols):
        l, s = divmod(c, 14)
        assert np.array_equal(Wp[:, 16 * l + s], W[:, c])
        if g.link_pos[l] >= 0:
            assert np.array_equal(Wc[:, 16 * int(g.link_pos[l]) + s], W[:, c])
        else:
            assert not W[:, c].any()
        if not extra:
            for compact in (False, True):
                buf, ldw = g.force_compact(compact)
                ldf, half = g.force_ld(compact), 3 * g.Nb
                F, T = buf[:half * ldf].reshape(half, ldf), buf[half * ldf:].reshape(half, ldw)
                p = int(g.link_pos[l]) if compact else l
                if p >= 0:
                    assert np.array_equal(T[:, 16 * p + s], W[half:, c])
                if 6 <= s < 10 and p >= 0:
                    assert np.array_equal(F[:, 16 * (p // 4) + 4 * (p % 4) + s - 6], W[:half, c])
    assert np.array_equal(qg.read_wrench_layout(W, g.rows, g.ncols, g.ncols), W)
    Wp = g.padded()
    assert np.array_equal(qg.read_wrench_layout(Wp, g.rows, g.ncols, Wp.shape[1], 16), W)
    Wc = g.padded(compact=True)
    assert Wc.shape[1] == 16 * g.nlive
    assert np.array_equal(qg.read_wrench_layout(Wc, g.rows, g.ncols, Wc.shape[1], 16, g.link_pos), W)
    if not extra:
        for compact in (False, True):
            buf, ldw = g.force_compact(compact)
            ldf = g.force_ld(compact)
            assert buf.size == 3 * g.Nb * (ldf + ldw)
            back = qg.read_wrench_layout(buf, g.rows, g.ncols, ldw, 16, g.link_pos if compact else None, ldf)
            assert np.array_equal(back, W)


def _blocks_generator(deps=True, with_inactive=True):
    import qr_graded_common as qg
    rng = np.random.default_rng(41)
    groups = [(2, [0, 1, 2, 3]), (5, [1, 2]), (7, [2]), (4, [3]), (3, [1])]
    return qg.RowBlocks(rng, 50, 6, groups, -20, 20, inactive=[5] if with_inactive else [], deps=deps,
                        noise={0: "tiny", 1: "big", 2: "mid", 3: "tiny"}, k_block=1)


def test_row_block_generator_lists_layouts_and_residual_identity():
    """tests/qr_graded_common.RowBlocks: every block is zero outside its list, the lists are what the matrix says, the
    dense and block-compact writers hold the same entries, the dependencies stay inside the blocks that list them, and
    ||tau_b - W_b phi||^2 = ||e_b||^2 exactly."""
    import qr_graded_common as qg
    g = _blocks_generator()
    assert g.counts.tolist()[5] == -1 and g.counts[4] == 0  # block 4: tau only; block 5: inactive
    for b in g.active():
        L = set(g.lists[b].tolist())
        outside = [c for c in range(g.n) if c not in L]
        assert not g.Mb(b)[:, outside].any()
        assert all(np.any(g.Mb(b)[:, c] != 0) for c in L)
    for b in g.active():  # the dependencies keep every column inside the blocks of its group
        assert np.array_equal(g.lists[b], np.flatnonzero(g.support[b]))
    R = np.linalg.qr(g.A()[:5 * g.rows_b], mode="r")
    assert len(g.dep) > 3 and (np.abs(np.diag(R))[g.dep] < 1e-9 * np.abs(np.diag(R)).max()).all()
    W = g.dense(16)
    flat, off, lds, local = g.compact()
    counts, cols, pos = g.block_columns(16)
    at = 0
    for b in range(g.nblocks):
        if counts[b] <= 0:
            continue
        Wb = flat[off[b]:off[b] + g.rows_b * lds[b]].reshape(g.rows_b, lds[b])
        c = slice(at, at + counts[b])
        assert np.array_equal(Wb[:, local[c]], W[b * g.rows_b:(b + 1) * g.rows_b][:, cols[c]])
        assert np.array_equal(pos[c], g.lists[b])
        at += counts[b]
    phi = g.phi()
    for b in g.active():
        sl = slice(b * g.rows_b, (b + 1) * g.rows_b)
        r = g.tau()[sl] - g.A()[sl] @ phi
        assert np.array_equal(r, g.e[sl])
    sq = [float(g.e[b * g.rows_b:(b + 1) * g.rows_b] @ g.e[b * g.rows_b:(b + 1) * g.rows_b]) for b in g.active()]
    assert max(sq) / min(sq) >= 2.0 ** 14  # (the GPU cases spread it over 2^30: 4096-row blocks)
    G = g.gram()
    for b in g.active():
        Gb = g.block_gram(b)
        L = np.r_[g.lists[b], g.n]
        v = np.r_[phi, -1.0][L]
        assert float(np.asarray(v, dtype=np.longdouble) @ np.asarray(Gb, dtype=np.longdouble) @ v) == sq[g.active().index(b)]
    assert np.diag(G).min() > 0
    assert np.array_equal(g.stack_offsets(), np.r_[0, np.cumsum([max(c + 1, 0) for c in g.counts])])  # (inactive: no rows)


def test_structured_planted_errors_rejected_columnwise_and_per_block():
    """Planted errors in a per-block triangle stack built with LAPACK: a 1e-9 relative error in the rows of a small-scale
    block, and in a small block's r^2.  The suite's older checks (|S^T S - G| <= 1e-11 max |G| for the stack, 1e-9 max
    sigma^2 for the variances) accept them; the per-block column-wise checks of test_qr_structured_graded.py reject them."""
    import qr_graded_common as qg
    g = _blocks_generator(deps=False, with_inactive=False)
    bexp = np.zeros(g.nblocks, dtype=np.int64)
    bexp[0] = -12  # block 0: rows at a small scale (exact: a power of two)
    nc = g.n + 1
    off = g.stack_offsets()
    S = np.zeros((int(off[-1]), nc))
    e2, Gb = [], {}
    for b in g.active():
        L = np.r_[g.lists[b], g.n]
        sl = slice(b * g.rows_b, (b + 1) * g.rows_b)
        Rb = np.linalg.qr(np.c_[g.A()[sl][:, g.lists[b]], g.tau()[sl]] * 2.0 ** bexp[b], mode="r")
        S[off[b]:off[b + 1], L] = Rb
        Gb[b] = g.block_gram(b) * 4.0 ** bexp[b]
        e2.append(float(g.e[sl] @ g.e[sl]) * 4.0 ** bexp[b])
    e2 = np.array(e2)
    G = np.asarray(g.gram(block_exp=bexp), dtype=np.float64)
    v = np.r_[g.phi(), -1.0]
    r2 = np.array([float(((S[off[b]:off[b + 1]] @ v) ** 2).sum()) for b in g.active()])

    from test_qr_structured_graded import C_R2, TOL_BACKWARD  # (the tolerances the GPU tests apply)

    def per_block(S):  # the backward metric of the GPU test's stack check, block by block
        return max(qg.backward_err(S[off[b]:off[b + 1]][:, np.r_[g.lists[b], g.n]], Gb[b]) for b in g.active())

    def r2_ok(r2):  # the GPU test's per-block residual check
        return all(qg.residual_ratio(r2[i], e2[i], np.r_[g.phi()[g.lists[b]], -1.0], Gb[b]) <= C_R2
                   for i, b in enumerate(g.active()))

    assert per_block(S) <= TOL_BACKWARD and r2_ok(r2)  # clean: both pass
    Sp = S.copy()
    Sp[off[0]:off[1]] *= 1.0 + 1e-9
    assert np.abs(Sp.T @ Sp - G).max() <= 1e-11 * np.abs(G).max()
    assert per_block(Sp) > TOL_BACKWARD
    r2p = r2.copy()
    small = int(np.argmin(e2))
    r2p[small] *= 1.0 + 1e-9
    assert np.abs(r2p - e2).max() <= 1e-9 * e2.max()
    assert not r2_ok(r2p)


# ------------------------------------------------------------------ column norms and residual sums (test_reductions_graded.py)
def test_reductions_colsq_ld_against_fractions():
    """tests/reductions_common.colsq_ld (long-double column sums of squares, in row chunks) against exact rational sums of
    the same float64 entries: relative error below m 2^-63 per column, whatever the chunking."""
    from fractions import Fraction

    import qr_graded_common as qg
    import reductions_common as rc
    qg.check_longdouble()  # (the 1e-300 entry and the m 2^-63 bound need an 80-bit long double)
    rng = np.random.default_rng(11)
    W = rng.standard_normal((53, 7)) * np.ldexp(1.0, rng.integers(-40, 40, 7))
    W[:, 3] = 0.0
    W[-1, 3] = 1e-300  # (the square underflows to a subnormal in float64, not in long double)
    for chunk in (1, 10, 53, 1000):
        got = rc.colsq_ld(W, chunk=chunk)
        for j in range(7):
            want = sum(Fraction(float(x)) ** 2 for x in W[:, j])
            assert abs(Fraction(*got[j].as_integer_ratio()) - want) <= Fraction(53 * 2.0 ** -63) * want
    assert rc.colsq_ld(np.zeros((4, 2))).tolist() == [0.0, 0.0]


def test_reductions_gamma_and_ratio():
    """gamma_m = m u / (1 - m u); colsq_ratio: a zero reference needs an exact zero, otherwise relative error / gamma_m."""
    import reductions_common as rc
    u = 2.0 ** -53
    assert rc.gamma(1) == u / (1 - u)
    assert rc.gamma(6 * 10 ** 6) == pytest.approx(6e6 * u, rel=1e-9)
    assert 1e-9 > rc.gamma(6 * 10 ** 6)  # (the margin of the straddling inputs beats gamma_m up to 6e6 rows)
    with pytest.raises(AssertionError):
        rc.gamma(2 ** 52)
    ref = np.array([0.0, 1.0, 2.0], dtype=np.longdouble)
    assert rc.colsq_ratio([0.0, 1.0, 2.0], ref, 10).max() == 0.0
    assert rc.colsq_ratio([1e-300, 1.0, 2.0], ref, 10)[0] == np.inf
    r = rc.colsq_ratio([0.0, 1.0 + 4 * u, 2.0], ref, 10)
    assert r[1] == pytest.approx(4 * u / rc.gamma(10), rel=1e-6) and r[1] < 1
    assert rc.colsq_ratio([0.0, 1.0 + 2e-15, 2.0], ref, 10)[1] > 1


@pytest.mark.parametrize("cfg", ["cfg2_ur10", "cfg4_talos"])
def test_reductions_straddle_builder_lands_where_claimed(cfg):
    """tests/reductions_common.straddle: inputs scaled so that the long-double sum of squares of their float64 values is
    tol_e (1 +- 1e-9) land on the claimed side with the claimed margin in the columns oracle_np.build_regressor_basic
    puts them in -- Ia of link k is a[:, k], fv is v[:, k], on row block k (joint torques) or on all six component rows
    (external wrench)."""
    from conftest import Golden

    import reductions_common as rc
    g = Golden(cfg)
    flat = g.flat()
    wrench = bool(g.param["is_external_wrench"])
    N = 8 if wrench else 300
    rng = np.random.default_rng(7)
    q = np.repeat(g["q_big"][:1], N, axis=0)
    v, a = rng.uniform(-2, 2, (N, int(flat["nv"]))), rng.uniform(-5, 5, (N, int(flat["nv"])))
    param = dict(g.param, has_friction=True, has_actuator_inertia=True, has_joint_offset=False)
    tol = 1e-6
    claims = {}
    for i, k in enumerate([0, 2, 3, 5]):
        x, slot, side = (a, 10, -1) if i % 2 == 0 else (v, 11, 1)
        side = side if i < 2 else -side
        x[:, k], _ = rc.straddle(x[:, k], tol, side, factor=6 if wrench else 1)
        claims[14 * k + slot] = side
    W = oracle_np.build_regressor_basic(flat, q, v, a, param)
    cs = rc.colsq_ld(W)
    for c, side in claims.items():
        rel = float((cs[c] - np.longdouble(tol)) / np.longdouble(tol))
        assert side * rel >= 0.99e-9 and abs(rel) <= 1.01e-9, "column %d: %.3e" % (c, rel)
    idx_e, kept = rc.exact_split(cs, tol)
    assert {c for c, s in claims.items() if s < 0} <= set(idx_e) and {c for c, s in claims.items() if s > 0} <= set(kept)


def test_reductions_planted_errors_rejected():
    """Planted errors the older checks accept and the new ones reject: (1) a column-norm vector within 1e-12 of its largest
    entry of the reference, but with one column moved across tol_e; (2) a sigma2_joint whose most precise joint is off by
    1e-3 relative, within 1e-9 of the largest variance."""
    import reductions_common as rc
    # (1) TX40-like spread: max colsq 2.95e7, one column at 0.9 tol_e moved to 1.1 tol_e (2e-7 < 1e-12 * 2.95e7 = 3e-5)
    tol = 1e-6
    ref = np.array([2.95e7, 3.1e2, 0.9 * tol, 0.0, 1.7], dtype=np.longdouble)
    cs = np.asarray(ref, dtype=np.float64).copy()
    cs[2] = 1.1 * tol
    assert rc.normwise_colsq_ok(cs, ref)
    assert rc.colsq_ratio(cs, ref, 6 * 400).max() > 1
    assert rc.exact_split(cs, tol)[0] != rc.exact_split(ref, tol)[0]
    cs_zero = np.asarray(ref, dtype=np.float64).copy()
    cs_zero[3] = 5e-6  # (a zero column reported at 5e-6: kept instead of eliminated)
    assert rc.normwise_colsq_ok(cs_zero, ref) and rc.colsq_ratio(cs_zero, ref, 2400)[3] == np.inf
    # (2) six joints, noise 1e-6 .. 1e-1 of a unit torque scale: sigma2 from 1e-12 to 1e-2
    rng = np.random.default_rng(4)
    N, nb = 500, 3
    Wb = rng.standard_normal((6 * N, nb))
    phi = rng.standard_normal(nb)
    lev = np.logspace(-6, -1, 6)
    tau = Wb @ phi + np.repeat(lev, N) * rng.standard_normal(6 * N)
    y = np.asarray(Wb, dtype=np.longdouble) @ np.asarray(phi, dtype=np.longdouble)
    sig2_ref = rc.sigma2_ld(tau, y, [N] * 6)
    bound = rc.sigma2_direct_bound(tau, Wb, phi, [N] * 6, np.sqrt(sig2_ref * N))
    sig2 = np.asarray(sig2_ref, dtype=np.float64)
    assert (np.abs(sig2 - sig2_ref) <= bound).all()  # the float64 rounding of the reference itself passes
    sig2[0] *= 1 + 1e-3
    assert np.abs(sig2 - np.asarray(sig2_ref, dtype=np.float64)).max() <= 1e-9 * float(sig2_ref.max())
    assert not (np.abs(sig2 - sig2_ref) <= bound).all()
