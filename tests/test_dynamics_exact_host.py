"""CPU tests of tests/dynamics_exact.py and of the host side of the inverse-dynamics mirrors.

(a) ``rnea_body_form`` -- the algorithm of csrc/figh_dynamics.hip in float64 NumPy -- against the long-double W . phi, row by
    row in units of u T: the largest ratio is C_TAU_ORACLE.  Measured here (N = 32, no flags and all flags, the model's own
    phi and a random signed one): TX40 2.1, UR10 4.2, TIAGo 9.4 (static, signed phi), TALOS 6.5, human 6.8; random trees 3.9 ..
    7.8 (largest: 13-link chain under a free-flyer, static).  Exact zeros wherever T == 0 in every case.
(b) C_TAU = 8 C_TAU_ORACLE rounded up to a power of two = 128.
(c) the metric catches planted errors (ratios in u T, C_TAU = 128; UR10, TIAGo, TALOS): w x (w x h) dropped 1.2e14 .. 2.1e14
    (regime fast); child wrench without its lever p x f 4.5e14 .. 2.4e15 (unit); the spatial-momentum form on TIAGo in regime
    fast 1.3e3 where the body form has 0.97 (it forms v_lin x (m v_lin), zero only analytically).
(d) host logic of the mirrors, with the device product replaced by NumPy on the oracle's W.
(e) figh_regressor_apply refuses to compute without a device.
"""
import numpy as np
import pytest

import dynamics_exact as dx
import oracle_np
import regressor_exact as rx

MODELS = ["tx40", "ur10", "tiago", "talos", "human"]
N_HOST = 32
FLAGS_ON = dict(friction=True, inertia=True, offset=True)


def _tree_flat(shape, freeflyer):
    from test_regressor_exact_host import _tree_flat as tree_flat
    return tree_flat(shape, freeflyer)


def _cases():
    from test_gpu_parity import _TREES
    cases = [(m, m) for m in MODELS]
    for shape in sorted(_TREES):
        cases += [(shape, shape), (shape + "-ff", shape)]
    return cases


def _flat_param(label, what, **flags):
    if label in MODELS:
        return rx.shipped_flat(label), rx.base_param(wrench=label in ("talos", "human"), **flags)
    ff = label.endswith("-ff")
    return _tree_flat(what, ff), rx.base_param(wrench=ff, **flags)


# ------------------------------------------------------------------------------------------------ (a), (b)
@pytest.mark.parametrize("label,what", _cases())
def test_body_form_within_scale(label, what):
    worst = 0.0
    for flags in ({}, FLAGS_ON):
        flat, param = _flat_param(label, what, **flags)
        nl = int(flat["njoints"]) - 1
        coupling = label == "tx40"
        pp = dx.drive_param(param, nl)
        phis = {"own": dx.phi_of(flat, pp, coupling), "signed": dx.phi_of(flat, pp, coupling, np.random.default_rng(nl))}
        for regime in rx.REGIMES:
            q, v, a = rx.inputs(flat, N_HOST, regime)
            ref = rx.regressor_ld(flat, q, v, a, param, coupling)
            for name, phi in phis.items():
                tau_ld, T = dx.tau_from_ref(ref, phi)
                r = dx.tau_ratio(dx.rnea_body_form(flat, q, v, a, phi, param, coupling), tau_ld, T)
                print("body form %-14s %-7s %-6s flags %d ratio %.2f" % (label, regime, name, bool(flags), r.ratio))
                assert r.zeros_ok, (label, regime, name)
                worst = max(worst, r.ratio)
    assert worst <= dx.C_TAU_ORACLE and 8 * worst <= dx.C_TAU, (label, worst)


def test_tolerance_constants():
    assert 8 * dx.C_TAU_ORACLE <= dx.C_TAU < 16 * dx.C_TAU_ORACLE and np.log2(dx.C_TAU) == int(np.log2(dx.C_TAU))


def test_zero_rows_are_exact():
    """phi zero except for one link's block: T vanishes on every row that is not of an ancestor of the link, and the body
    form returns exact zeros there."""
    flat = rx.shipped_flat("tiago")
    param = rx.base_param()
    q, v, a = rx.inputs(flat, 8, "unit")
    ref = rx.regressor_ld(flat, q, v, a, param)
    depth = [0] * int(flat["njoints"])
    for j in range(1, int(flat["njoints"])):
        depth[j] = depth[int(flat["parents"][j])] + 1
    k = int(np.argmax(depth)) - 1  # (0-based link: the deepest one)
    phi = np.zeros(ref.W.shape[1])
    phi[14 * k:14 * k + 10] = dx.phi_of(flat, param)[14 * k:14 * k + 10]
    tau_ld, T = dx.tau_from_ref(ref, phi)
    anc, j = set(), k + 1
    while j > 0:
        anc.add(j - 1)
        j = int(flat["parents"][j])
    live = (T.reshape(-1, 8) > 0).any(axis=1)
    assert set(np.flatnonzero(live)) == anc and 1 < len(anc) < int(flat["nv"])
    r = dx.tau_ratio(dx.rnea_body_form(flat, q, v, a, phi, param), tau_ld, T)
    assert r.zeros_ok and r.ratio <= dx.C_TAU_ORACLE
    bad = dx.rnea_body_form(flat, q, v, a, phi, param)
    bad[np.flatnonzero(T == 0)[0]] = 1e-300
    assert not dx.tau_ratio(bad, tau_ld, T).zeros_ok


# ------------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("model", ["ur10", "tiago", "talos"])
def test_planted_errors(model):
    flat, param = _flat_param(model, model)
    phi = dx.phi_of(flat, param)
    for name, regime, kw in (("centripetal", "fast", dict(drop="centripetal")), ("lever", "unit", dict(drop="lever"))):
        q, v, a = rx.inputs(flat, N_HOST, regime, seed=5)
        tau_ld, T = dx.tau_from_ref(rx.regressor_ld(flat, q, v, a, param), phi)
        good = dx.tau_ratio(dx.rnea_body_form(flat, q, v, a, phi, param), tau_ld, T).ratio
        bad = dx.tau_ratio(dx.rnea_body_form(flat, q, v, a, phi, param, **kw), tau_ld, T).ratio
        print("planted %-12s %-6s %-5s good %.2f bad %.3g (C_TAU %g)" % (name, model, regime, good, bad, dx.C_TAU))
        assert good <= dx.C_TAU_ORACLE
        assert bad > dx.C_TAU, (name, bad)


def test_spatial_momentum_form_is_rejected():
    flat, param = _flat_param("tiago", "tiago")
    phi = dx.phi_of(flat, param)
    q, v, a = rx.inputs(flat, N_HOST, "fast")
    tau_ld, T = dx.tau_from_ref(rx.regressor_ld(flat, q, v, a, param), phi)
    body = dx.tau_ratio(dx.rnea_body_form(flat, q, v, a, phi, param), tau_ld, T).ratio
    mom = dx.tau_ratio(dx.rnea_body_form(flat, q, v, a, phi, param, form="momentum"), tau_ld, T)
    print("TIAGo fast: body form %.2f, spatial-momentum form %.3g u T (row %s)" % (body, mom.ratio, mom.worst))
    assert body <= dx.C_TAU_ORACLE
    assert mom.ratio > dx.C_TAU


# ------------------------------------------------------------------------------------------------------ (d)
def _robot(name):
    from figaroh_plus_amd.tools.robot import Robot
    return Robot.from_flat(name)


@pytest.fixture
def numpy_product(monkeypatch):
    """The device product of the mirrors replaced by NumPy on the oracle's W; returns the list of the calls made."""
    from figaroh_plus_amd.tools import regressor
    calls = []

    class Host:
        def __init__(self, x):
            self.x = x

        def to_host(self):
            return self.x.copy()

    def fake(robot, q, v, a, param, phi, coupling):
        flat = robot.model.to_flat()
        W = oracle_np.build_regressor_basic(flat, q, v, a, param)
        if coupling:
            W = oracle_np.add_coupling_TX40(W, len(q), v, a)
        calls.append(dict(N=len(q), param=dict(param), coupling=coupling, phi=np.array(phi)))
        return Host(W @ phi)

    monkeypatch.setattr(regressor, "_times_parameters", fake)
    return calls


@pytest.mark.parametrize("name", ["ur10", "tiago", "talos"])
def test_parameter_vector_order(name):
    """get_standard_parameters is the column order of the regressor: its values are dynamics_exact.phi_of's."""
    robot = _robot(name)
    flat = robot.model.to_flat()
    nl = robot.model.njoints - 1
    param = dx.drive_param(rx.base_param(wrench=name == "talos", **FLAGS_ON), nl)
    std = robot.get_standard_parameters(param)
    assert list(std)[:14] == ["Ixx1", "Ixy1", "Ixz1", "Iyy1", "Iyz1", "Izz1", "mx1", "my1", "mz1", "m1", "Ia1", "fv1", "fs1", "off1"]
    assert np.array_equal(np.array(list(std.values()), dtype=float), dx.phi_of(flat, param))
    off = robot.get_standard_parameters(dict(param, has_friction=False))
    assert all(off["fv%d" % k] == 0 and off["fs%d" % k] == 0 for k in range(1, nl + 1))


def test_cols_scatter(numpy_product):
    from figaroh_plus_amd.tools.excitation import base_columns
    from figaroh_plus_amd.tools.regressor import expand_parameters, regressor_times_parameters
    robot = _robot("ur10")
    flat = robot.model.to_flat()
    param = rx.base_param(**FLAGS_ON)
    q, v, a = rx.inputs(flat, 20, "unit")
    W = oracle_np.build_regressor_basic(flat, q, v, a, param)
    idx_e = [0, 1, 2, 3, 4, 6, 7, 9, 14, 16]
    kept = [c for c in range(84) if c not in idx_e]
    idx_base = [0, 2, 5, 11, 30, 44, 73]
    cols = base_columns(84, idx_e, idx_base)
    assert cols.tolist() == [kept[i] for i in idx_base]
    phi_b = np.random.default_rng(1).standard_normal(len(cols))
    tau = regressor_times_parameters(robot, q, v, a, param, phi_b, cols=cols)
    assert np.array_equal(tau, W @ expand_parameters(phi_b, 84, cols))
    assert np.abs(tau - W[:, cols] @ phi_b).max() <= 1e-12 * np.abs(tau).max()
    full = numpy_product[-1]["phi"]
    assert np.array_equal(full[cols], phi_b) and np.count_nonzero(full) == len(cols)
    for bad_phi, bad_cols in ((phi_b[:-1], cols), (phi_b, list(cols[:-1]) + [84]), (phi_b, list(cols[:-1]) + [int(cols[0])]),
                              (np.zeros(83), None)):
        with pytest.raises(ValueError):
            regressor_times_parameters(robot, q, v, a, param, bad_phi, cols=bad_cols)
    with pytest.raises(ValueError):
        regressor_times_parameters(robot, q, v, a, param, np.zeros(84), coupling=True)  # 87 columns with the coupling


def _reference_get_torque_rand(N, rnea, nv, v, a, param):
    """The statements of src/figaroh/tools/randomdata.py:106-146 with pin.rnea replaced by ``rnea`` (N x nv)."""
    tau = np.zeros(nv * N)
    for i in range(N):
        for j in range(nv):
            tau[j * N + i] = rnea[i, j]
    if param["has_friction"]:
        for i in range(N):
            for j in range(nv):
                tau[j * N + i] += v[i, j] * param["fv"][j] + np.sign(v[i, j]) * param["fs"][j]
    if param["has_actuator_inertia"]:
        for i in range(N):
            for j in range(nv):
                tau[j * N + i] += param["Ia"][j] * a[i, j]
    if param["has_joint_offset"]:
        for i in range(N):
            for j in range(nv):
                tau[j * N + i] += param["off"][j]
    if param["has_coupled_wrist"]:
        for i in range(N):
            for j in range(nv):
                s = np.sign(v[i, nv - 2] + v[i, nv - 1])
                if j == nv - 2:
                    tau[j * N + i] += param["Iam6"] * v[i, nv - 1] + param["fvm6"] * v[i, nv - 1] + param["fsm6"] * s
                if j == nv - 1:
                    tau[j * N + i] += param["Iam6"] * v[i, nv - 2] + param["fvm6"] * v[i, nv - 2] + param["fsm6"] * s
    return tau


@pytest.mark.parametrize("flags", range(16))
def test_get_torque_rand_flag_blocks(flags, numpy_product):
    from figaroh_plus_amd.tools.randomdata import get_torque_rand
    robot = _robot("tx40")
    flat = robot.model.to_flat()
    N, nv = 12, 6
    param = dx.drive_param(dict(rx.base_param(), has_friction=bool(flags & 1), has_actuator_inertia=bool(flags & 2),
                                has_joint_offset=bool(flags & 4), has_coupled_wrist=bool(flags & 8)), nv)
    q, v, a = rx.inputs(flat, N + 3, "one")  # (sign(0) = 0 in most entries; three samples more than N: only N are used)
    rigid = rx.base_param()
    rnea = (oracle_np.build_regressor_basic(flat, q[:N], v[:N], a[:N], rigid) @ dx.phi_of(flat, rigid)).reshape(nv, N).T
    want = _reference_get_torque_rand(N, rnea, nv, v, a, param)
    tau = get_torque_rand(N, robot, q, v, a, param)
    call = numpy_product[-1]
    assert call["N"] == N and call["coupling"] is False and call["param"]["is_joint_torques"]
    assert tau.shape == (nv * N,)
    assert np.abs(tau - want).max() <= 1e-13 * np.abs(want).max()
    if flags & 8:  # Iam6 multiplies a VELOCITY in the reference (randomdata.py:130): not the regressor's coupling columns
        Wc = oracle_np.add_coupling_TX40(oracle_np.build_regressor_basic(flat, q[:N], v[:N], a[:N], param), N, v[:N], a[:N])
        coupled = Wc @ dx.phi_of(flat, param, coupling=True)
        assert np.abs(coupled - want).max() > 1e-3


def test_calc_torque_and_batch_reshaping(numpy_product):
    from figaroh_plus_amd.tools.excitation import calc_torque, calc_torque_batch, split_batch
    robot = _robot("ur10")
    flat = robot.model.to_flat()
    B, n_per, nv = 3, 7, 6
    param = dx.drive_param(rx.base_param(**FLAGS_ON), nv)  # (friction and the like are not part of calc_torque)
    trajs = [rx.inputs(flat, n_per, "unit", seed=b) for b in range(B)]
    rigid = rx.base_param()
    phi = dx.phi_of(flat, rigid)
    singles = []
    for q, v, a in trajs:
        tau = calc_torque(n_per, robot, q, v, a, param)
        assert numpy_product[-1]["param"]["has_friction"] is False and not numpy_product[-1]["phi"][10:14].any()
        assert np.array_equal(tau, oracle_np.build_regressor_basic(flat, q, v, a, rigid) @ phi)
        singles.append(tau)
    ncalls = len(numpy_product)
    out = calc_torque_batch(robot, trajs, param)
    assert len(numpy_product) == ncalls + 1 and numpy_product[-1]["N"] == B * n_per  # one product for the whole batch
    assert out.shape == (B, nv * n_per)
    assert np.abs(out - np.array(singles)).max() <= 1e-13 * np.abs(out).max()
    t = np.arange(nv * B * n_per, dtype=float)
    s = split_batch(t, B, nv, n_per)
    for b in range(B):
        for j in range(nv):
            assert np.array_equal(s[b, j * n_per:(j + 1) * n_per], j * B * n_per + b * n_per + np.arange(n_per))
    with pytest.raises(ValueError):
        calc_torque_batch(robot, [trajs[0], tuple(x[:-1] for x in trajs[1])], param)
    with pytest.raises(ValueError):
        calc_torque_batch(robot, [], param)


def test_launch_rule_matches_the_kernel_source():
    """_lib.APPLY_WAVES_PER_CU states csrc/figh_dynamics.hip's kDynWavesPerCu (the GPU tests size their persistent-grid cases
    by it)."""
    import os
    import re
    from conftest import ROOT
    from figaroh_plus_amd import _lib
    with open(os.path.join(ROOT, "figaroh_plus_amd", "csrc", "figh_dynamics.hip")) as f:
        m = re.search(r"constexpr int kDynWavesPerCu = (\d+);", f.read())
    assert m and int(m.group(1)) == _lib.APPLY_WAVES_PER_CU


# ------------------------------------------------------------------------------------------------------ (e)
def test_apply_fails_loudly_without_gpu():
    import __graft_entry__ as entry
    import os
    from figaroh_plus_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    rc = _lib.load().figh_regressor_apply(None, _lib.MODE_JOINT_TORQUE, 0, 63, 4, None, None, None, None, None)
    assert rc == _lib.ERR_NO_DEVICE
    assert b"no HIP device" in _lib.load().figh_last_error()
    from figaroh_plus_amd.tools.regressor import regressor_times_parameters
    robot = _robot("ur10")
    with pytest.raises(_lib.FighError) as e:
        regressor_times_parameters(robot, np.zeros((4, 6)), np.zeros((4, 6)), np.zeros((4, 6)), rx.base_param(), np.zeros(84))
    assert e.value.code == _lib.ERR_NO_DEVICE
