"""CPU suite: the excitation-trajectory mirror (figaroh_plus_amd/tools/excitation.py: CubicSpline, spline_*,
waypoints_from_search_variables, constraint_vector) against the scalar emulation and the 50-digit reference of
tests/trajectory_common.py.  ndcurves is not a dependency: parity with the reference's generator is mathematical (the same
quintic), checked to rounding against exact arithmetic, entry by entry, |mirror - exact| <= C_SPLINE 2^-53 S."""
import numpy as np
import pytest

import trajectory_common as tc

# largest |mirror - exact| / (2^-53 S) observed: 2.66 over HOST_CASES (printed by test_mirror_and_emulation_against_exact), 2.73
# over the GPU suite's shapes (test_gpu_shapes_mirror_and_emulation_against_exact, `unequal_one`)


def _spline(name="ur10_all", n_wps=4):
    robot, make, q0 = tc.model_case(name)
    return robot, make(n_wps), q0


@pytest.fixture(scope="module")
def host_cases():
    """Per case: inputs, emulation, mirror and exact reference of a six-joint trajectory, computed once."""
    robot, make, _ = tc.model_case("ur10_all")
    out = {}
    for n, (tag, tps, freq) in enumerate(tc.HOST_CASES):
        rng = np.random.default_rng(10 + n)
        wps, vel, acc = tc.waypoint_set(rng, 6, len(tps))
        t, q, dq, ddq = tc.spline_emul(freq, tps, wps, vel, acc)
        ref, S = tc.spline_exact(tps, wps, vel, acc, t)
        cs = make(len(tps))
        mirror = cs.get_active_config(freq, np.array(tps).reshape(-1, 1), wps, vel, acc)
        out[tag] = dict(tps=tps, freq=freq, wps=wps, vel=vel, acc=acc, t=t, emul=(q, dq, ddq), ref=ref, S=S, mirror=mirror,
                        spline=cs)
    return out


def test_mirror_and_emulation_against_exact(host_cases):
    worst = 0.0
    for tag, c in host_cases.items():
        t, p, v, a = c["mirror"]
        assert t.shape == (len(c["t"]), 1) and np.array_equal(t[:, 0], c["t"])
        for got, want in zip((p, v, a), c["emul"]):
            assert np.array_equal(got, want), tag  # bit-equal: the same operations in the same order
        ratio = tc.worst_ratio(np.stack(c["emul"]), c["ref"], c["S"])
        print("%s: largest |mirror - exact| / (2^-53 S) = %.2f" % (tag, ratio))
        assert ratio <= tc.C_SPLINE, (tag, ratio)
        worst = max(worst, ratio)
    print("largest ratio over the cases %.2f (C_SPLINE = %g)" % (worst, tc.C_SPLINE))


@pytest.fixture(scope="module")
def shape_cases():
    """The shapes of the GPU suite (tc.gpu_shapes(): n_wps 2, 3, 10, magnitudes scaled by 2^+-20, n_per below, at and above
    the reference's N, so that the cap on u is exercised) and its 100-waypoint case, on UR10's six joints with the GPU suite's
    seeds: first trajectory of each batch, emulation, package mirror and exact reference computed once.  The 100-waypoint
    case is compared with exact arithmetic at every 37th sample and at the last one (mpmath is slow)."""
    shapes = [(tag, tps, freq, n_per, B, per, scale, 1000 + n, None)
              for n, (tag, tps, freq, n_per, B, per, scale) in enumerate(tc.gpu_shapes())]
    shapes.append(("hundred", [0.5 * i for i in range(100)], 100, 4951, 1, False, 1.0, 4, sorted(set(range(0, 4951, 37)) | {4950})))
    out = {}
    for tag, tps, freq, n_per, B, per, scale, seed, sub in shapes:
        wps, vel, acc = tc.waypoint_set(np.random.default_rng(seed), 6, len(tps), scale, B=B)
        wps, vel, acc = wps[0], vel[0], acc[0]
        t, q, dq, ddq = tc.spline_emul(freq, tps, wps, vel, acc, n_per=n_per)
        emul = np.stack((q, dq, ddq))
        sub = np.arange(n_per) if sub is None else np.array(sub)
        ref, S = tc.spline_exact(tps, wps, vel, acc, t[sub])
        out[tag] = dict(tps=tps, freq=freq, n_per=n_per, wps=wps, vel=vel, acc=acc, t=t, emul=emul, sub=sub, ref=ref, S=S)
    return out


def test_gpu_shapes_mirror_and_emulation_against_exact(shape_cases):
    """Every shape the kernels are compared with the emulation on: the emulation is within C_SPLINE 2^-53 S of exact
    arithmetic entry by entry, and the package mirror is bit-equal to it -- the samples past tps[-1] included."""
    from figaroh_plus_amd.tools.excitation import spline_coefficients, spline_samples, spline_times
    worst, capped = 0.0, 0
    for tag, c in shape_cases.items():
        _, _, N, t, k, u = spline_times(c["freq"], c["tps"], n_per=c["n_per"])
        assert N == tc.sample_times(c["freq"], c["tps"])[0] and np.array_equal(t, c["t"])
        mirror = np.stack(spline_samples(spline_coefficients(c["tps"], c["wps"], c["vel"], c["acc"]), k, u))
        assert np.array_equal(mirror, c["emul"]), tag
        capped += int(np.sum(t > c["tps"][-1]))
        ratio = tc.worst_ratio(c["emul"][:, c["sub"]], c["ref"], c["S"])
        print("%s: n_wps %d, n_per %d (N %d): largest |mirror - exact| / (2^-53 S) = %.2f" % (tag, len(c["tps"]), c["n_per"], N, ratio))
        assert ratio <= tc.C_SPLINE, (tag, ratio)
        worst = max(worst, ratio)
    assert capped > 0, "no shape samples past the last time point: the cap on u is not exercised"
    past = shape_cases["freq7_past_the_end"]
    end = past["t"] > past["tps"][-1]  # behind the end: the end conditions of the last waypoint, to the scale
    assert end.sum() >= 30 and np.all(past["emul"][:, end] == past["emul"][:, end][:, :1])
    print("largest ratio over the shapes %.2f (C_SPLINE = %g)" % (worst, tc.C_SPLINE))


@pytest.mark.parametrize("tag,plant", [("on_waypoints", "c4"), ("on_waypoints", "segment"), ("on_waypoints_big", "c4"),
                                       ("on_waypoints_big", "segment"), ("freq7_tiny", "c4"), ("freq7_past_the_end", "c4"),
                                       ("unequal", "c4"), ("one_segment", "c4"), ("hundred", "c4"), ("hundred", "segment")])
def test_planted_errors_are_caught_on_gpu_shapes(shape_cases, tag, plant):
    c = shape_cases[tag]
    _, q, dq, ddq = tc.spline_emul(c["freq"], c["tps"], c["wps"], c["vel"], c["acc"], n_per=c["n_per"], plant=plant)
    planted = np.stack((q, dq, ddq))
    assert not np.array_equal(planted, c["emul"])
    assert tc.worst_ratio(planted[:, c["sub"]], c["ref"], c["S"]) > tc.C_SPLINE


def test_sample_count_and_time_column(host_cases):
    for tag, c in host_cases.items():
        cs, tps, freq = c["spline"], c["tps"], c["freq"]
        delta_t = 1 / freq
        N = int((tps[-1] - tps[0]) / delta_t) + 1
        t = c["mirror"][0]
        assert cs.N == N == len(t) and cs.delta_t == delta_t and cs.T == tps[-1] - tps[0]
        assert isinstance(t, np.ndarray) and t.shape == (N, 1)
        assert np.array_equal(t[:, 0], np.array([tps[0] + i * delta_t for i in range(N)]))
    assert host_cases["on_waypoints"]["spline"].N == 13 and host_cases["freq7"]["spline"].N == 15


def test_samples_on_and_off_waypoints(host_cases):
    from figaroh_plus_amd.tools.excitation import waypoint_sample_indices
    c = host_cases["on_waypoints"]
    assert list(waypoint_sample_indices(c["mirror"][0], c["tps"])) == [4, 8, 12]
    c = host_cases["unequal"]
    assert len(waypoint_sample_indices(c["mirror"][0], c["tps"])) == 0
    literal = []  # optimal_trajectory.py:157-162
    c = host_cases["freq7"]
    t_f, time_points = c["mirror"][0], np.array(c["tps"]).reshape(-1, 1)[range(1, 5), :]
    for i in range(t_f.shape[0]):
        if t_f[i, 0] in time_points:
            literal.append(i)
    assert list(waypoint_sample_indices(t_f, c["tps"])) == literal


def test_end_conditions_and_continuity(host_cases):
    """Position, velocity and acceleration waypoints are met at both ends of every segment to the error scale: the end of
    segment k (u = h) and the start of segment k + 1 (u = 0) give the same three values, so the spline is C2."""
    for tag, c in host_cases.items():
        tps, wps, vel, acc = c["tps"], c["wps"], c["vel"], c["acc"]
        for s in range(wps.shape[0]):
            for k in range(len(tps) - 1):
                h = tps[k + 1] - tps[k]
                coef = tc.segment_coefficients(h, *(float(x) for x in (wps[s, k], wps[s, k + 1], vel[s, k], vel[s, k + 1],
                                                                      acc[s, k], acc[s, k + 1])))
                start, end = tc.horner(coef, 0.0), tc.horner(coef, h)
                assert start == (wps[s, k], vel[s, k], acc[s, k])  # c0, c1, 2 (a0 / 2): exact
                _, S = tc.spline_exact(tps[k:k + 2], wps[s:s + 1, k:k + 2], vel[s:s + 1, k:k + 2], acc[s:s + 1, k:k + 2],
                                       [tps[k + 1]])
                for d, want in enumerate((wps[s, k + 1], vel[s, k + 1], acc[s, k + 1])):
                    assert abs(end[d] - want) <= tc.C_SPLINE * tc.EPS * float(S[d, 0, 0]), (tag, s, k, d)


def test_midpoint_of_a_rest_to_rest_segment():
    """Zero velocity / acceleration waypoints: the 10-15-6 profile, whose midpoint is (p0 + p1) / 2."""
    rng = np.random.default_rng(3)
    tps = [0.0, 0.75, 2.0]
    wps, vel, acc = tc.waypoint_set(rng, 6, 3, zero_rates=True)
    robot, cs, _ = _spline(n_wps=3)
    from figaroh_plus_amd.tools.excitation import spline_coefficients, spline_samples
    coef = spline_coefficients(tps, wps, vel, acc)
    for k in range(2):
        h = tps[k + 1] - tps[k]
        q, dq, ddq = spline_samples(coef, np.array([k]), np.array([h / 2]))
        _, S = tc.spline_exact(tps, wps, vel, acc, [tps[k] + h / 2])
        for s in range(6):
            assert abs(q[0, s] - (wps[s, k] + wps[s, k + 1]) / 2) <= tc.C_SPLINE * tc.EPS * float(S[0, 0, s])
            assert abs(ddq[0, s]) <= tc.C_SPLINE * tc.EPS * float(S[2, 0, s])  # the acceleration changes sign there


@pytest.mark.parametrize("plant", ["c4", "segment"])
def test_planted_errors_are_caught(host_cases, plant):
    """A wrong constant in c4, or the segment index off by one at the samples that sit on a waypoint."""
    c = host_cases["on_waypoints"]
    t, q, dq, ddq = tc.spline_emul(c["freq"], c["tps"], c["wps"], c["vel"], c["acc"], plant=plant)
    assert not np.array_equal(q, c["emul"][0])
    assert tc.worst_ratio(np.stack((q, dq, ddq)), c["ref"], c["S"]) > tc.C_SPLINE


def test_full_config_scatter():
    for name in tc.MODEL_CASES:
        robot, cs, q0 = _spline(name, 3)
        rng = np.random.default_rng(5)
        n_act = len(cs.act_idxq)
        wps, vel, acc = tc.waypoint_set(rng, n_act, 3)
        tps = np.array([[0.0], [0.5], [1.0]])
        t, p, v, a = cs.get_full_config(8, tps, wps, vel, acc)
        _, q_e, dq_e, ddq_e = tc.spline_emul(8, tps, wps, vel, acc)
        want = tc.full_config_emul(q0, robot.model.nv, cs.act_idxq, cs.act_idxv, q_e, dq_e, ddq_e)
        for got, w in zip((p, v, a), want):
            assert got.shape == w.shape and np.array_equal(got, w), name
        assert cs.dim_q == (n_act, 3) and cs.dim_v == (n_act, 3)
        assert cs.act_idxq == [robot.model.joints[j].idx_q for j in cs.act_Jid]
    robot, cs, _ = _spline("tiago_arm", 3)
    assert cs.act_idxq != cs.act_idxv and robot.model.nq != robot.model.nv


def test_limits_and_soft_limits():
    from figaroh_plus_amd.tools.excitation import CubicSpline
    robot, cs, _ = _spline()
    m = robot.model
    assert np.array_equal(cs.upper_q, m.upperPositionLimit) and np.array_equal(cs.lower_dq, -m.velocityLimit)
    soft = CubicSpline(robot, 4, tc.MODEL_CASES["ur10_all"][1], soft_lim=0.05)
    up = m.upperPositionLimit - 0.05 * abs(m.upperPositionLimit - m.lowerPositionLimit)
    lo = m.lowerPositionLimit + 0.05 * abs(up - m.lowerPositionLimit)  # (the reference's statement order)
    assert np.array_equal(soft.upper_q, up) and np.array_equal(soft.lower_q, lo)
    up = m.effortLimit - 0.05 * abs(2 * m.effortLimit)
    assert np.array_equal(soft.upper_effort, up) and np.array_equal(soft.lower_effort, -m.effortLimit + 0.05 * abs(up + m.effortLimit))


def test_check_cfg_constraints(capsys):
    robot, cs, _ = _spline()
    m = robot.model
    q = np.zeros((3, 6))
    assert cs.check_cfg_constraints(q, np.zeros((3, 6)), np.zeros((3, 6))) is False
    assert "SUCCEEDED" in capsys.readouterr().out
    q[1, 2] = m.upperPositionLimit[2] + 1.0
    assert cs.check_cfg_constraints(q) is True
    out = capsys.readouterr().out
    assert "Joint q 2 upper limit violated!" in out and "FAILED to generate a feasible cubic spline" in out
    v = np.zeros((3, 6))
    v[0, 4] = -2 * m.velocityLimit[4]
    assert cs.check_cfg_constraints(np.zeros((3, 6)), v) is True
    assert "Joint vel idx_v 4 limits violated!" in capsys.readouterr().out


def test_assertions_and_refusals():
    robot, cs, _ = _spline()
    rng = np.random.default_rng(1)
    wps, vel, acc = tc.waypoint_set(rng, 6, 4)
    tps = np.array([[0.0], [0.5], [1.0], [1.5]])
    pad = " " * 40
    with pytest.raises(AssertionError) as e:
        cs.get_active_config(10, tps, wps[:, :3], vel, acc)
    assert str(e.value) == "(Pos) Check size " + pad + "(num_active_joints,num_waypoints)!"
    with pytest.raises(AssertionError) as e:
        cs.get_active_config(10, tps, wps, vel[:5], acc)
    assert str(e.value) == "(Vel) Check size" + pad + "(num_active_joints, num_waypoints)!"
    with pytest.raises(AssertionError) as e:
        cs.get_full_config(10, tps, wps, vel, acc.T)
    assert str(e.value) == "(Acc) Check size" + pad + "(num_active_joints, num_waypoints)!"
    with pytest.raises(NotImplementedError, match="ndcurves"):
        cs.get_active_config(10, tps, wps)
    with pytest.raises(NotImplementedError, match="ndcurves"):
        cs.get_full_config(10, tps, wps, vel, None, device_resident=True)
    for bad in ([0.0, 0.5, 0.5, 1.0], [0.0, 1.0, 0.5, 1.5], [0.0, 0.5, 1.0, np.inf]):
        with pytest.raises(ValueError, match="strictly increasing"):
            cs.get_active_config(10, np.array(bad).reshape(-1, 1), wps, vel, acc)
    from figaroh_plus_amd.tools.excitation import CubicSpline, spline_batch
    tiago = tc.model_case("tiago_arm")[0]
    wheel = CubicSpline(tiago, 4, ["wheel_left_joint", "arm_1_joint"])  # a continuous joint: (cos, sin)
    human = tc.model_case("human_arms")[0]
    root = CubicSpline(human, 4, ["root_joint"])
    for spline, n in ((wheel, 2), (root, 1)):
        w, v, a = tc.waypoint_set(rng, n, 4)
        with pytest.raises(ValueError, match="not one revolute or prismatic degree of freedom"):
            spline.get_active_config(10, tps, w, v, a)
        with pytest.raises(ValueError, match="not one revolute or prismatic degree of freedom"):
            spline_batch(spline, 10, tps, w[None], v, a)
    with pytest.raises(ValueError, match="wps_batch"):
        spline_batch(cs, 10, tps, wps, vel, acc)


def test_waypoints_from_search_variables():
    from figaroh_plus_amd.tools.excitation import waypoints_from_search_variables
    rng = np.random.default_rng(2)
    n_wps, active_joints = 5, list(range(8))
    wp_init = rng.normal(size=8)
    X_batch = rng.normal(size=(7, (n_wps - 1) * 8))
    got = waypoints_from_search_variables(X_batch, wp_init, n_wps, 8)
    assert got.shape == (7, 8, n_wps) and got.flags["C_CONTIGUOUS"]
    for b in range(7):
        X = np.array(list(X_batch[b]))  # optimal_trajectory.py:116-119
        wps_X = np.reshape(X, (n_wps - 1, len(active_joints)))
        wps = np.vstack((wp_init, wps_X))
        wps = wps.transpose()
        assert np.array_equal(got[b], wps)


def test_constraint_vector_ordering():
    """constraint_vector -- the host form that constraints_batch's kernel is compared with on the GPU -- against the literal
    statements of optimal_trajectory.py:156-174, :185-187."""
    from figaroh_plus_amd.tools.excitation import constraint_vector
    robot, CB, _ = _spline("tiago_arm", 4)
    rng = np.random.default_rng(4)
    n_wps = 4
    tps = np.array([[0.0], [0.5], [1.0], [1.5]])
    wps, vel, acc = tc.waypoint_set(rng, 8, n_wps)
    t_f, p_f, v_f, a_f = CB.get_full_config(8, tps, wps, vel, acc)
    Ns = p_f.shape[0]
    tau = rng.normal(size=robot.model.nv * Ns)
    idx_waypoints = []
    time_points = tps[range(1, n_wps), :]
    for i in range(t_f.shape[0]):
        if t_f[i, 0] in time_points:
            idx_waypoints.append(i)
    q_constraints = p_f[idx_waypoints, :]
    q_constraints = q_constraints[:, CB.act_idxq]
    v_constraints = v_f[:, CB.act_idxv]
    tau_constraints = np.zeros((Ns, len(CB.act_idxv)))
    for k in range(len(CB.act_idxv)):
        tau_constraints[:, k] = tau[range(CB.act_idxv[k] * Ns, (CB.act_idxv[k] + 1) * Ns)]
    constr_vec = np.concatenate((q_constraints, v_constraints, tau_constraints), axis=None)
    assert idx_waypoints == [4, 8, 12]
    got = constraint_vector(CB, t_f, p_f, v_f, tau, tps)
    assert got.shape == (3 * 8 + 2 * Ns * 8,) and np.array_equal(got, constr_vec)


def test_entries_fail_loudly_without_gpu():
    """Without a HIP device both entries answer FIGH_ERR_NO_DEVICE before they look at an argument (with one, the NULL
    arguments are refused)."""
    import os
    import __graft_entry__ as entry
    from figaroh_plus_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    lib = _lib.load()
    want = _lib.ERR_NO_DEVICE if _lib.device_count() == 0 else _lib.ERR_INVALID
    assert lib.figh_spline_sample(None, 1, 2, 1, 2, 100.0, None, None, None, None, None, 0, None, 0, None, None, 6, None, None,
                                  6) == want
    assert lib.figh_excitation_constraints(None, 1, 2, 1, None, None, 0, None, None, 6, None, 6, None, None, 4) == want
    if want == _lib.ERR_NO_DEVICE:
        assert b"no HIP device" in lib.figh_last_error()
        robot, cs, _ = _spline()
        wps, vel, acc = tc.waypoint_set(np.random.default_rng(0), 6, 4)
        with pytest.raises(_lib.FighError) as e:
            cs.get_full_config(10, [0.0, 0.5, 1.0, 1.5], wps, vel, acc, device_resident=True)
        assert e.value.code == _lib.ERR_NO_DEVICE
