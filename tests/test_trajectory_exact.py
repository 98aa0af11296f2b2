"""GPU suite: figh_spline_sample and figh_excitation_constraints (csrc/figh_trajectory.hip) and the Python layer on top of
them.  The kernels are compared BIT FOR BIT with the scalar emulation of tests/trajectory_common.py (whose distance from the
exact quintic the CPU suite bounds); every output is pre-filled with the module's sentinel and has spare rows and a padded
leading dimension, which are asserted untouched.  End to end, a resident TrajectoryBatch gives what the list form of the same
arrays gives, and one evaluate_waypoints_batch moves no sample array across the bus."""
import numpy as np
import pytest

import trajectory_common as tc
from conftest import Golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    return _lib


def _sentinel(lib, rows, ld):
    return lib.DeviceArray.from_host(np.full(rows * ld, tc.SENTINEL))


def _run_raw(lib, robot, cs, q0, tps, freq, n_per, wps, vel, acc):
    """figh_spline_sample through _lib on sentinel-filled, padded buffers: (q, v, a) as written, checked outside."""
    m = robot.model
    B = wps.shape[0]
    rows, ldq, ldv = B * n_per, m.nq + 3, m.nv + 1
    d_q, d_v, d_a = _sentinel(lib, rows + 2, ldq), _sentinel(lib, rows + 2, ldv), _sentinel(lib, rows + 2, ldv)
    d = [lib.DeviceArray.from_host(np.ascontiguousarray(x).reshape(-1)) for x in (wps, vel, acc)]
    stride = [0 if x.ndim == 2 else x.shape[1] * x.shape[2] for x in (vel, acc)]
    d_q0 = lib.DeviceArray.from_host(q0)
    lib.spline_sample(robot.device_model(), B, len(tps), n_per, freq, cs.act_idxq, cs.act_idxv, tps, d[0], d[1], stride[0],
                      d[2], stride[1], d_q0, d_q.ptr, ldq, d_v.ptr, d_a.ptr, ldv)
    out = []
    for buf, ld, width in ((d_q, ldq, m.nq), (d_v, ldv, m.nv), (d_a, ldv, m.nv)):
        full = buf.to_host().reshape(rows + 2, ld)
        assert np.all(full[:rows, width:] == tc.SENTINEL) and np.all(full[rows:] == tc.SENTINEL)
        out.append(full[:rows, :width])
    return out


def _want(robot, cs, q0, tps, freq, n_per, wps, vel, acc):
    parts = []
    for b in range(wps.shape[0]):
        _, q, dq, ddq = tc.spline_emul(freq, tps, wps[b], vel if vel.ndim == 2 else vel[b], acc if acc.ndim == 2 else acc[b],
                                       n_per=n_per)
        parts.append(tc.full_config_emul(q0, robot.model.nv, cs.act_idxq, cs.act_idxv, q, dq, ddq))
    return [np.concatenate([p[k] for p in parts]) for k in range(3)]


def _compare(robot, cs, got, want, tag):
    for g, w, what in zip(got, want, "qva"):
        assert np.array_equal(g, w), (tag, what, np.argwhere(g != w)[:5])
    quiet = np.ones(robot.model.nv, dtype=bool)
    quiet[cs.act_idxv] = False
    for g in got[1:]:  # inactive columns: +0.0, bit for bit
        assert np.all(g[:, quiet] == 0.0) and not np.any(np.signbit(g[:, quiet]))


@pytest.mark.parametrize("name", list(tc.MODEL_CASES))
def test_spline_sample_bit_equal_to_emulation(lib, name):
    robot, make, q0 = tc.model_case(name)
    for n, (tag, tps, freq, n_per, B, per_traj, scale) in enumerate(tc.gpu_shapes()):
        cs = make(len(tps))
        n_act = len(cs.act_idxq)
        rng = np.random.default_rng(1000 + n)
        wps, vel, acc = tc.waypoint_set(rng, n_act, len(tps), scale, B=B)
        if not per_traj:  # one set of velocity / acceleration waypoints for the batch (stride 0)
            vel, acc = vel[0], acc[0]
        got = _run_raw(lib, robot, cs, q0, tps, freq, n_per, wps, vel, acc)
        _compare(robot, cs, got, _want(robot, cs, q0, tps, freq, n_per, wps, vel, acc), (name, tag))


def test_spline_sample_hundred_waypoints(lib):
    """get_idx_b_cubic's shape: 100 waypoints half a second apart at 100 Hz, 4951 samples; and the rest-to-rest form of the
    script (zero velocity / acceleration waypoints) through CubicSpline itself."""
    robot, make, q0 = tc.model_case("ur10_all")
    tps = [0.5 * i for i in range(100)]
    cs = make(100)
    rng = np.random.default_rng(4)
    wps, vel, acc = tc.waypoint_set(rng, 6, 100, B=1)
    got = _run_raw(lib, robot, cs, q0, tps, 100, 4951, wps, vel[0], acc[0])
    _compare(robot, cs, got, _want(robot, cs, q0, tps, 100, 4951, wps, vel[0], acc[0]), "hundred")
    from figaroh_plus_amd.device import GpuMatrix
    from figaroh_plus_amd.tools.excitation import waypoint_sample_indices
    zero = np.zeros((6, 100))
    t, p, v, a = cs.get_full_config(100, np.array(tps).reshape(-1, 1), wps[0], zero, zero, device_resident=True)
    assert cs.N == 4951 and t.shape == (4951, 1) and all(isinstance(x, GpuMatrix) for x in (p, v, a))
    th, ph, vh, ah = cs.get_full_config(100, np.array(tps).reshape(-1, 1), wps[0], zero, zero)
    assert np.array_equal(t, th)
    for g, w in zip((p, v, a), (ph, vh, ah)):
        assert np.array_equal(g.numpy(), w)  # device and NumPy mirror: bit-equal
    idx = waypoint_sample_indices(t, tps)
    idx = idx[t[idx, 0] < tps[-1]]  # (a sample on an interior waypoint starts its segment: u = 0, the position is c0)
    assert len(idx) > 50 and np.array_equal(ph[idx][:, cs.act_idxq], wps[0][:, np.searchsorted(tps, t[idx, 0])].T)


def test_more_trajectories_than_grid_rows(lib):
    """B = 65537 trajectories of two samples: the kernels walk the trajectories on a grid dimension of at most 65535 and
    loop over the rest.  Reference: the package mirror (bit-equal to the emulation, CPU suite) and host slicing."""
    from figaroh_plus_amd.tools import excitation as ex
    robot, make, q0 = tc.model_case("ur10_two")
    cs, m = make(3), robot.model
    B, n_per, tps = 65537, 2, [0.0, 0.5, 1.0]
    wps, vel, acc = tc.waypoint_set(np.random.default_rng(12), 2, 3, B=B)
    q, v, a = _run_raw(lib, robot, cs, q0, tps, 1.5, n_per, wps, vel, acc)
    _, _, _, t, k, u = ex.spline_times(1.5, tps, n_per=n_per)
    assert list(k) == [0, 1]
    mirror = ex.spline_samples(ex.spline_coefficients(tps, wps, vel, acc), k, u)  # each (B, n_per, 2)
    for got, idx, want in ((q, cs.act_idxq, mirror[0]), (v, cs.act_idxv, mirror[1]), (a, cs.act_idxv, mirror[2])):
        assert np.array_equal(got[:, idx], want.reshape(B * n_per, 2))
    quiet = np.ones(m.nq, dtype=bool)
    quiet[cs.act_idxq] = False
    assert np.array_equal(q[:, quiet], np.broadcast_to(q0[quiet], (B * n_per, quiet.sum())))
    tau = np.random.default_rng(13).normal(size=m.nv * B * n_per)
    n_con = 2 + 2 * n_per * 2
    d_q, d_v, d_tau = (lib.DeviceArray.from_host(np.ascontiguousarray(x).reshape(-1)) for x in (q, v, tau))
    d_out = _sentinel(lib, B + 1, n_con)
    lib.excitation_constraints(robot.device_model(), B, n_per, cs.act_idxq, cs.act_idxv, [1], d_q.ptr, m.nq, d_v.ptr, m.nv, d_tau,
                               d_out.ptr, n_con)
    out = d_out.to_host().reshape(B + 1, n_con)
    assert np.all(out[B] == tc.SENTINEL)
    qb, vb, tb = q.reshape(B, n_per, m.nq), v.reshape(B, n_per, m.nv), tau.reshape(m.nv, B, n_per)
    want = np.concatenate((qb[:, 1][:, cs.act_idxq], vb[:, :, cs.act_idxv].reshape(B, -1),
                           tb[cs.act_idxv].transpose(1, 2, 0).reshape(B, -1)), axis=1)
    assert np.array_equal(out[:B], want)
    for b in (0, 65535, 65536):  # and the literal statements on the rows either side of the grid's end
        assert np.array_equal(out[b], ex.constraint_vector(cs, np.array([0.0, 0.5]), qb[b], vb[b], tb[:, b].reshape(-1), [0.0, 0.5]))


def _constraints_want(cs, q, v, tau, B, n_per, idx):
    """Host slicing, trajectory by trajectory (optimal_trajectory.py:156-174, :185-187)."""
    nv = v.shape[1]
    rows = []
    for b in range(B):
        p_f, v_f = q[b * n_per:(b + 1) * n_per], v[b * n_per:(b + 1) * n_per]
        q_c = p_f[idx, :][:, cs.act_idxq]
        v_c = v_f[:, cs.act_idxv]
        tau_b = tau.reshape(nv, B, n_per)[:, b, :].reshape(-1)  # calc_torque's layout of trajectory b
        tau_c = np.zeros((n_per, len(cs.act_idxv)))
        for k in range(len(cs.act_idxv)):
            tau_c[:, k] = tau_b[range(cs.act_idxv[k] * n_per, (cs.act_idxv[k] + 1) * n_per)]
        rows.append(np.concatenate((q_c, v_c, tau_c), axis=None))
    return np.array(rows)


@pytest.mark.parametrize("name", ["ur10_two", "tiago_arm"])
def test_excitation_constraints_bit_equal_to_host_slicing(lib, name):
    robot, make, _ = tc.model_case(name)
    cs = make(4)
    m = robot.model
    n_act = len(cs.act_idxq)
    rng = np.random.default_rng(9)
    for B, n_per, idx in ((1, 2, []), (3, 45, [0, 44]), (3, 63, [7, 21, 62]), (1, 65, [64]), (3, 257, [64, 128, 256])):
        rows, ldq, ldv = B * n_per, m.nq + 2, m.nv + 3
        q, v = np.full((rows, ldq), np.nan), np.full((rows, ldv), np.nan)
        q[:, :m.nq], v[:, :m.nv] = rng.normal(size=(rows, m.nq)), rng.normal(size=(rows, m.nv))
        tau = rng.normal(size=m.nv * rows)
        n_con = len(idx) * n_act + 2 * n_per * n_act
        ld_out = n_con + 2
        d_q, d_v, d_tau = (lib.DeviceArray.from_host(x.reshape(-1)) for x in (q, v, tau))
        d_out = _sentinel(lib, B + 1, ld_out)
        lib.excitation_constraints(robot.device_model(), B, n_per, cs.act_idxq, cs.act_idxv, idx, d_q.ptr, ldq, d_v.ptr, ldv,
                                   d_tau, d_out.ptr, ld_out)
        out = d_out.to_host().reshape(B + 1, ld_out)
        assert np.all(out[:B, n_con:] == tc.SENTINEL) and np.all(out[B] == tc.SENTINEL)
        want = _constraints_want(cs, q[:, :m.nq], v[:, :m.nv], tau, B, n_per, idx)
        assert np.array_equal(out[:B, :n_con], want), (name, B, n_per)


# ------------------------------------------------------------------------------------------------------------ end to end
def _problem(cfg, case, tps, B, seed):
    g = Golden(cfg)
    robot, make, _ = tc.model_case(case)
    cs = make(len(tps))
    n_act, n_wps = cs.dim_q
    rng = np.random.default_rng(seed)
    wp_init = rng.uniform(-0.5, 0.5, size=n_act)
    X = rng.uniform(-1.0, 1.0, size=(B, (n_wps - 1) * n_act))
    vel, acc = 0.3 * rng.normal(size=(n_act, n_wps)), rng.normal(size=(n_act, n_wps))
    return g, robot, cs, wp_init, X, vel, acc


def _indices_from_spline(robot, make, param):
    """get_idx_b_cubic / get_idx_from_random (optimal_trajectory.py:43-53, :72-94) at a smaller size: the eliminated and the
    base columns of a random spline of the ACTIVE joints -- with the golden's indices, found on a motion of every joint, the
    base regressor of an arm-only trajectory is singular and its condition number says nothing."""
    from figaroh_plus_amd.tools.qrdecomposition import get_baseIndex
    from figaroh_plus_amd.tools.regressor import build_regressor_basic, build_regressor_reduced, get_index_eliminate
    cs = make(10)
    wps, vel, acc = tc.waypoint_set(np.random.default_rng(40), cs.dim_q[0], 10)
    _, p, v, a = cs.get_full_config(100, np.array([[0.5 * i] for i in range(10)]), wps, vel, acc)
    W = build_regressor_basic(robot, p, v, a, param)
    idx_e, par_r = get_index_eliminate(W, robot.get_standard_parameters(param), tol_e=0.001)
    return idx_e, get_baseIndex(build_regressor_reduced(W, idx_e), par_r)


@pytest.mark.parametrize("cfg,case,tps,B,n_per", [("cfg2_ur10", "ur10_all", [0.0, 0.5, 1.0, 1.295], 3, 130),
                                                  ("cfg3_tiago", "tiago_arm", [0.0, 0.25, 0.5, 0.895], 2, 90)])
def test_resident_batch_equals_list_form(lib, cfg, case, tps, B, n_per):
    from figaroh_plus_amd.tools import excitation as ex
    g, robot, cs, wp_init, X, vel, acc = _problem(cfg, case, tps, B, 21)
    param, idx_e, idx_base = dict(g.param), g["idx_e"], g["idx_base"]
    if case == "tiago_arm":
        idx_e, idx_base = _indices_from_spline(robot, tc.model_case(case)[1], param)
        assert 0 < len(idx_base) < len(g["idx_base"])
    wps = ex.waypoints_from_search_variables(X, wp_init, *cs.dim_q[::-1])
    batch = ex.spline_batch(cs, 100, tps, wps, vel, acc)
    assert (batch.B, batch.n_per) == (B, n_per) and batch.t.shape == (n_per, 1)
    lists = batch.numpy()
    for b in range(B):  # the resident samples are the NumPy mirror's
        _, p, v, a = cs.get_full_config(100, np.array(tps).reshape(-1, 1), wps[b], vel, acc)
        assert all(np.array_equal(x, y) for x, y in zip(lists[b], (p, v, a)))
    tau_list = ex.calc_torque_batch(robot, lists, param)
    tau_batch = ex.calc_torque_batch(robot, batch, param)
    assert tau_batch.shape == (B, robot.model.nv * n_per) and np.array_equal(tau_batch, tau_list)
    d_tau = ex.calc_torque_batch(robot, batch, dict(param, device_resident=True))
    assert isinstance(d_tau, lib.DeviceArray)
    assert np.array_equal(ex.split_batch(d_tau.to_host(), B, robot.model.nv, n_per), tau_list)
    cond_list = ex.objective_cond_batch(robot, lists, param, idx_e, idx_base)
    cond_batch = ex.objective_cond_batch(robot, batch, param, idx_e, idx_base)
    for got, ref in zip(cond_batch, cond_list):
        print("%s: cond resident %.12g list %.12g" % (cfg, got, ref))
        assert abs(got - ref) <= 1e-9 * ref
    cons = ex.constraints_batch(cs, batch, d_tau, tps)
    want = np.array([ex.constraint_vector(cs, batch.t, *lists[b][:2], tau_list[b], tps) for b in range(B)])
    assert cons.shape == want.shape and np.array_equal(cons, want)
    conds, cons2 = ex.evaluate_waypoints_batch(robot, cs, 100, tps, X, vel, acc, wp_init, param, idx_e, idx_base)
    assert np.array_equal(cons2, cons)
    for got, ref in zip(conds, cond_list):
        assert abs(got - ref) <= 1e-9 * ref


def test_evaluate_waypoints_batch_moves_no_sample_array(lib, monkeypatch):
    """One evaluate_waypoints_batch of 8 x 1000 UR10 samples: no upload or download of B n_per entries or more, except the
    (B, n_con) result and the B r x r triangles."""
    from figaroh_plus_amd.tools import excitation as ex
    tps = [0.0, 2.5, 5.0, 7.5, 9.995]
    B = 8
    g, robot, cs, wp_init, X, vel, acc = _problem("cfg2_ur10", "ur10_all", tps, B, 22)
    up, down = [], []
    from_host, to_host = lib.DeviceArray.from_host.__func__, lib.DeviceArray.to_host

    def rec_up(cls, arr, dtype=None):
        up.append(int(np.asarray(arr).size))
        return from_host(cls, arr, dtype)

    def rec_down(self, out=None):
        down.append(self.size)
        return to_host(self, out)

    def no_matrix_download(self):
        raise AssertionError("GpuMatrix.numpy() inside the resident route (it copies through figh_memcpy_d2h itself)")

    from figaroh_plus_amd.device import GpuMatrix
    monkeypatch.setattr(lib.DeviceArray, "from_host", classmethod(rec_up))
    monkeypatch.setattr(lib.DeviceArray, "to_host", rec_down)
    monkeypatch.setattr(GpuMatrix, "numpy", no_matrix_download)
    conds, cons = ex.evaluate_waypoints_batch(robot, cs, 100, tps, X, vel, acc, wp_init, dict(g.param), g["idx_e"], g["idx_base"])
    monkeypatch.undo()
    n_per, r = 1000, len(g["idx_base"])
    n_con = 6 * len(ex.waypoint_sample_indices(ex.spline_times(100, tps)[3], tps)) + 2 * n_per * 6
    assert len(conds) == B and cons.shape == (B, n_con)
    assert up and max(up) < B * n_per, up
    assert sorted(x for x in down if x >= B * n_per) == sorted([B * n_con, B * r * r]), down


def test_refusals_launch_nothing(lib):
    robot, make, q0 = tc.model_case("tiago_arm")
    m = robot.model
    cs = make(3)
    rng = np.random.default_rng(8)
    wps, vel, acc = tc.waypoint_set(rng, 8, 3, B=2)
    n_per = 9
    d = [lib.DeviceArray.from_host(x.reshape(-1)) for x in (wps, vel, acc)]
    d_q0 = lib.DeviceArray.from_host(q0)
    d_q, d_v, d_a = _sentinel(lib, 2 * n_per, m.nq), _sentinel(lib, 2 * n_per, m.nv), _sentinel(lib, 2 * n_per, m.nv)
    wheel = m.joints[m.getJointId("wheel_left_joint")]

    def call(tps=(0.0, 0.5, 1.0), idxq=cs.act_idxq, idxv=cs.act_idxv, stride=24, ldq=m.nq):
        lib.spline_sample(robot.device_model(), 2, 3, n_per, 8, idxq, idxv, np.array(tps), d[0], d[1], stride, d[2], stride,
                          d_q0, d_q.ptr, ldq, d_v.ptr, d_a.ptr, m.nv)

    cases = [("tps equal", dict(tps=(0.0, 0.5, 0.5)), lib.ERR_INVALID), ("tps back", dict(tps=(0.0, 1.0, 0.5)), lib.ERR_INVALID),
             ("stride", dict(stride=23), lib.ERR_INVALID), ("ldq", dict(ldq=m.nq - 1), lib.ERR_INVALID),
             ("no joint", dict(idxq=[cs.act_idxq[0] + 1] + cs.act_idxq[1:]), lib.ERR_INVALID),
             ("twice", dict(idxq=cs.act_idxq[:7] + cs.act_idxq[:1], idxv=cs.act_idxv[:7] + cs.act_idxv[:1]), lib.ERR_INVALID),
             ("continuous", dict(idxq=[wheel.idx_q] + cs.act_idxq[1:], idxv=[wheel.idx_v] + cs.act_idxv[1:]), lib.ERR_UNSUPPORTED)]
    lib.profile_enable(level=2)
    try:
        lib.profile_reset()
        for tag, kw, code in cases:
            with pytest.raises(lib.FighError) as e:
                call(**kw)
            assert e.value.code == code, tag
        assert "revolute or prismatic" in str(e.value)
        human, hmake, hq0 = tc.model_case("human_arms")
        root = human.model.joints[1]
        h_out = [_sentinel(lib, n_per, 64) for _ in range(3)]
        with pytest.raises(lib.FighError) as e:
            lib.spline_sample(human.device_model(), 1, 3, n_per, 8, [root.idx_q], [root.idx_v], np.array([0.0, 0.5, 1.0]), d[0],
                              d[1], 0, d[2], 0, lib.DeviceArray.from_host(hq0), h_out[0].ptr, 64, h_out[1].ptr, h_out[2].ptr, 64)
        assert e.value.code == lib.ERR_UNSUPPORTED and all(np.all(b.to_host() == tc.SENTINEL) for b in h_out)
        d_tau, d_out = lib.DeviceArray.from_host(np.zeros(m.nv * 2 * n_per)), _sentinel(lib, 2, 2 * n_per * 8 + 8)
        for idx, idxq, code in (([n_per], cs.act_idxq, lib.ERR_INVALID), ([-1], cs.act_idxq, lib.ERR_INVALID),
                                ([0], [wheel.idx_q] + cs.act_idxq[1:], lib.ERR_INVALID)):
            with pytest.raises(lib.FighError) as e:
                lib.excitation_constraints(robot.device_model(), 2, n_per, idxq, cs.act_idxv, idx, d_q.ptr, m.nq, d_v.ptr,
                                           m.nv, d_tau, d_out.ptr, 2 * n_per * 8 + 8)
            assert e.value.code == code
        assert lib.profile_get("spline_sample")[0] == 0 and lib.profile_get("excitation_constraints")[0] == 0
        assert all(np.all(b.to_host() == tc.SENTINEL) for b in (d_q, d_v, d_a, d_out))
        call()  # (every buffer has the size this shape asks for)
        assert lib.profile_get("spline_sample")[0] == 1 and not np.any(d_q.to_host() == tc.SENTINEL)
    finally:
        lib.profile_enable(False)
