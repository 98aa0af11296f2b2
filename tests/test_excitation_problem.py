"""GPU suite: figh_difference_quotients (csrc/figh_trajectory.hip) bit for bit against its NumPy statement, and
tools.excitation.ExcitationProblem end to end: its Jacobian is the quotient of the rows that evaluate_waypoints_batch returns
for the same host-made stencil, its condition numbers stay within the singular values' bound of the host route, one
derivative pass moves no batch-sized array but the Jacobian, and the four methods at one X launch one pass."""
import functools

import numpy as np
import pytest

import singular_common as sc
import trajectory_common as tc
from figaroh_plus_amd.tools import excitation as ex

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    return _lib


@pytest.mark.parametrize("scheme", ["2-point", "3-point"])
def test_difference_quotients_bit_equal(lib, scheme):
    """Every n_con of {1, 63, 64, 65, 1000} with every n_var of {1, 15, 16, 17, 72} (below, on and above the 32 x 32 tile,
    several tiles each way): padded ldc and ldj, sentinels in the padding, in spare rows of J and in the unused rows of C."""
    rng = np.random.default_rng(5)
    for n_con in (1, 63, 64, 65, 1000):
        for n_var in (1, 15, 16, 17, 72):
            B = 1 + n_var * (1 if scheme == "2-point" else 2)
            ldc, ldj = n_con + 3, n_var + 2
            C = np.full((B + 1, ldc), tc.SENTINEL)
            C[:B, :n_con] = rng.normal(size=(B, n_con)) * 10.0 ** rng.integers(-3, 4, size=(B, 1))
            dx = rng.uniform(1e-8, 1e-5, size=n_var) * rng.choice([-1.0, 1.0], size=n_var)
            d_C, d_dx = lib.DeviceArray.from_host(C.reshape(-1)), lib.DeviceArray.from_host(dx)
            d_J = lib.DeviceArray.from_host(np.full((n_con + 2) * ldj, tc.SENTINEL))
            lib.difference_quotients(d_C, ldc, n_con, n_var, ex.SCHEMES[scheme], d_dx, d_J, ldj)
            J = d_J.to_host().reshape(n_con + 2, ldj)
            assert np.all(J[:n_con, n_var:] == tc.SENTINEL) and np.all(J[n_con:] == tc.SENTINEL), (n_con, n_var)
            want = ex.difference_quotients(C[:B, :n_con], dx, scheme)
            assert np.array_equal(J[:n_con, :n_var], want), (n_con, n_var, np.argwhere(J[:n_con, :n_var] != want)[:5])
            assert np.array_equal(d_C.to_host(), C.reshape(-1))


def test_difference_quotients_refusals_launch_nothing(lib):
    d_C, d_dx = lib.DeviceArray.from_host(np.ones(3 * 4)), lib.DeviceArray.from_host(np.ones(2))
    d_J = lib.DeviceArray.from_host(np.full(4 * 2, tc.SENTINEL))

    def call(ldc=4, n_con=4, n_var=2, scheme=2, ldj=2):
        lib.difference_quotients(d_C, ldc, n_con, n_var, scheme, d_dx, d_J, ldj)

    lib.profile_enable(level=2)
    try:
        lib.profile_reset()
        for kw in (dict(scheme=1), dict(scheme=4), dict(n_var=0), dict(n_con=0), dict(ldc=3), dict(ldj=1)):
            with pytest.raises(lib.FighError) as e:
                call(**kw)
            assert e.value.code == lib.ERR_INVALID, kw
        assert lib.profile_get("difference_quotients")[0] == 0 and np.all(d_J.to_host() == tc.SENTINEL)
        call()
        assert lib.profile_get("difference_quotients")[0] == 1 and np.all(d_J.to_host() == 0.0)
    finally:
        lib.profile_enable(False)


# ------------------------------------------------------------------------------------------------------------ the problems
@functools.lru_cache(maxsize=None)
def _setup(name):
    """(robot, spline, tps, X, vel, acc, wp_init, param, idx_e, idx_base, collision) of the two problems: UR10, 5 waypoints,
    100 Hz, 200 samples; TIAGo's eight script joints with the collision fixture, 4 waypoints, 60 samples."""
    from conftest import Golden
    from test_trajectory_exact import _indices_from_spline, _problem
    if name == "ur10":
        tps = [0.0, 0.5, 1.0, 1.5, 1.995]
        g, robot, cs, wp_init, X, vel, acc = _problem("cfg2_ur10", "ur10_all", tps, 1, 31)
        return robot, cs, tps, X[0], vel, acc, wp_init, dict(g.param), g["idx_e"], g["idx_base"], None
    import collision_common as cc
    from figaroh_plus_amd.tools import robotcollisions as rc
    g = Golden("cfg3_tiago")
    robot = cc.tiago_case()
    robot.q0 = tc.model_case("tiago_arm")[2]
    joints = tc.MODEL_CASES["tiago_arm"][1]
    cs = ex.CubicSpline(robot, 4, joints)
    param = dict(g.param)
    idx_e, idx_base = _indices_from_spline(robot, lambda n: ex.CubicSpline(robot, n, joints), param)
    tps = [0.0, 0.2, 0.4, 0.6]
    rng = np.random.default_rng(32)
    n_act, n_wps = cs.dim_q
    wp_init = rng.uniform(-0.3, 0.3, size=n_act)
    lo, up = np.maximum(cs.lower_q, -1.5), np.minimum(cs.upper_q, 1.5)
    X = rng.uniform(np.tile(lo, n_wps - 1), np.tile(up, n_wps - 1))
    vel, acc = 0.3 * rng.normal(size=(n_act, n_wps)), rng.normal(size=(n_act, n_wps))
    return robot, cs, tps, X, vel, acc, wp_init, param, idx_e, idx_base, rc.CollisionWrapper(robot)


def _make(name, **kw):
    robot, cs, tps, X, vel, acc, wp_init, param, idx_e, idx_base, cw = _setup(name)
    return ex.ExcitationProblem(robot, cs, 100, tps, vel, acc, wp_init, param, idx_e, idx_base, collision=cw, **kw), X


@pytest.mark.parametrize("scheme", ["2-point", "3-point"])
@pytest.mark.parametrize("name", ["ur10", "tiago"])
def test_problem_jacobian_equals_batch_route(lib, name, scheme):
    robot, cs, tps, X, vel, acc, wp_init, param, idx_e, idx_base, cw = _setup(name)
    prob, _ = _make(name, scheme=scheme)
    assert prob.n_per == (200 if name == "ur10" else 61) and prob.n_var == 24
    J, c0 = prob.jacobian(X), prob.constraints(X)
    h, dx = ex.finite_difference_steps(X, scheme)
    stencil = ex.finite_difference_stencil(X, h, scheme)
    conds, rows = ex.evaluate_waypoints_batch(robot, cs, 100, tps, stencil, vel, acc, wp_init, param, idx_e, idx_base,
                                              collision=cw)
    assert rows.shape == (len(stencil), prob.n_con) and J.shape == (prob.n_con, prob.n_var)
    want = ex.difference_quotients(rows, dx, scheme)
    assert np.array_equal(J, want), np.argwhere(J != want)[:5]
    assert np.array_equal(c0, rows[0]) and np.array_equal(prob.last_pass.dx, dx)
    assert len(prob.bounds()[0]) == prob.n_var
    if name == "tiago":  # (every waypoint behind the first falls on a sample: the bounds of get_constr_value fit the rows)
        assert len(prob.idx_waypoints) == prob.n_wps - 1 and len(prob.constraint_bounds()[0]) == prob.n_con
    assert np.isfinite(J).all() and np.count_nonzero(J) > prob.n_var
    assert (prob.derivative_passes, prob.value_passes) == (1, 0)


@pytest.mark.parametrize("scheme", ["2-point", "3-point"])
@pytest.mark.parametrize("name", ["ur10", "tiago"])
def test_problem_conds_within_bound_of_host_route(lib, name, scheme):
    """|cond_dev - cond_host| <= 2 C_SV r 2^-53 cond_host^2: either route carries at most C_SV r 2^-53 sigma_max in sigma_min.
    The host route is LAPACK on the triangles of the same pass (downloaded here); the condition numbers of a second problem
    with singular_values="host", whose pass factors the samples again, are held to the same bound."""
    from figaroh_plus_amd._host import singular_values_batch
    prob, X = _make(name, scheme=scheme)
    grad = prob.gradient(X)
    p = prob.last_pass
    B, r, n = p.B, prob.r, prob.n_var
    assert p.host_fallbacks == 0 and p.sweeps.shape == (B,) and p.sweeps.max() <= sc.MAX_SWEEPS
    tri = np.triu(prob._pass_buffers(B)[3].to_host().reshape(B, r, r))
    s = singular_values_batch(tri)
    cond_host = s[:, 0] / s[:, -1]
    bound = 2 * sc.C_SV * r * 2.0 ** -53 * cond_host ** 2
    print("%s %s: r %d, cond %.6g, sweeps max %d, worst |dev - host| / bound %.3g"
          % (name, scheme, r, cond_host[0], p.sweeps.max(), (np.abs(p.conds - cond_host) / bound).max()))
    assert np.all(np.abs(p.conds - cond_host) <= bound)
    lo = p.conds[0] if scheme == "2-point" else p.conds[1 + n:]
    assert np.array_equal(grad, (p.conds[1:1 + n] - lo) / p.dx)
    assert np.array_equal(grad, ex.difference_quotients(p.conds[:, None], p.dx, scheme)[0])
    assert prob.objective(X) == p.conds[0] and prob.derivative_passes == 1
    host, _ = _make(name, scheme=scheme, singular_values="host")
    host.gradient(X)
    again = np.abs(p.conds - host.last_pass.conds) / bound
    print("%s %s: against a second pass on the host route: worst ratio %.3g" % (name, scheme, again.max()))
    assert host.last_pass.sweeps is None and np.all(again <= 1.0)


def test_derivative_pass_moves_no_batch_array(lib, monkeypatch):
    """One derivative pass of the UR10 problem (B = 25 trajectories of 200 samples): no upload or download of B n_per entries
    or more except the (n_con, n_var) Jacobian -- in particular no B r^2 and no B n_con download -- by the recording
    instrument of test_evaluate_waypoints_batch_moves_no_sample_array and, below it, by the bytes of every device-to-host
    copy the library is asked for."""
    from figaroh_plus_amd.device import GpuMatrix
    prob, X = _make("ur10")
    prob.objective(X + 0.01)  # (buffers of both pass sizes exist; the constants went up with the constructor)
    up, down, raw = [], [], []
    from_host, to_host = lib.DeviceArray.from_host.__func__, lib.DeviceArray.to_host
    d2h = lib.load().figh_memcpy_d2h

    def rec_up(cls, arr, dtype=None):
        up.append(int(np.asarray(arr).size))
        return from_host(cls, arr, dtype)

    def rec_down(self, out=None):
        down.append(self.size)
        return to_host(self, out)

    def rec_raw(dst, src, nbytes):
        raw.append(int(nbytes))
        return d2h(dst, src, nbytes)

    def no_matrix_download(self):
        raise AssertionError("GpuMatrix.numpy() inside the resident route")

    monkeypatch.setattr(lib.DeviceArray, "from_host", classmethod(rec_up))
    monkeypatch.setattr(lib.DeviceArray, "to_host", rec_down)
    monkeypatch.setattr(GpuMatrix, "numpy", no_matrix_download)
    monkeypatch.setattr(lib.load(), "figh_memcpy_d2h", rec_raw)
    J = prob.jacobian(X)
    monkeypatch.undo()
    B, n_per, r, n_con, n_var = prob.last_pass.B, prob.n_per, prob.r, prob.n_con, prob.n_var
    assert B == 25 and n_per == 200 and J.shape == (n_con, n_var) and prob.last_pass.host_fallbacks == 0
    assert B * r < B * n_per < n_con * n_var and n_con < B * n_per
    assert sorted(up) == sorted([B * 6 * 5, n_var]), up  # the stencil's waypoints and the steps
    assert sorted(down) == sorted([B * r, 2 * B, n_con * n_var, n_con]), down  # sigma, status, the Jacobian, row 0
    assert sorted(raw) == sorted(8 * x if x != 2 * B else 4 * x for x in down), raw
    assert B * r * r not in down and B * n_con not in down


def test_four_calls_one_pass(lib):
    """objective, gradient, constraints and jacobian at one X launch what one derivative pass launches: one launch of each
    family; a trial point then costs one value pass (no quotients), and its derivatives one more derivative pass."""
    prob, X = _make("tiago")
    families = ("spline_sample", "singular_values_batch", "excitation_constraints", "collision_distances", "difference_quotients")
    lib.profile_enable(level=2)
    try:
        lib.profile_reset()
        f, g, c, J = prob.objective(X), prob.gradient(X), prob.constraints(X), prob.jacobian(X)
        assert [lib.profile_get(k)[0] for k in families] == [1, 1, 1, 1, 1]
        assert (prob.derivative_passes, prob.value_passes) == (1, 0) and prob.last_pass.B == 1 + prob.n_var
        assert f == prob.last_pass.conds[0] and g.shape == (prob.n_var,) and c.shape == (prob.n_con,)
        X1 = X + 1e-3
        f1, c1 = prob.objective(X1), prob.constraints(X1)
        assert [lib.profile_get(k)[0] for k in families] == [2, 2, 2, 2, 1] and prob.value_passes == 1
        assert abs(f1 - f) <= 0.1 * f and np.abs(c1 - c).max() > 0
        prob.jacobian(X1), prob.gradient(X1), prob.objective(X1), prob.constraints(X1)
        assert [lib.profile_get(k)[0] for k in families] == [3, 3, 3, 3, 2] and prob.derivative_passes == 2
        # the value pass and row 0 of the derivative pass are the same trajectory: the same constraint row
        assert np.array_equal(prob.constraints(X1), c1)
    finally:
        lib.profile_enable(False)


def test_objective_cond_batch_device_route(lib):
    """objective_cond_batch(singular_values="device") on resident samples: within the bound of the default (host) route."""
    robot, cs, tps, X, vel, acc, wp_init, param, idx_e, idx_base, _ = _setup("ur10")
    Xs = np.stack([X, X + 0.01, X - 0.02, X + 0.03])
    wps = ex.waypoints_from_search_variables(Xs, wp_init, *cs.dim_q[::-1])
    batch = ex.spline_batch(cs, 100, tps, wps, vel, acc)
    host = np.array(ex.objective_cond_batch(robot, batch, param, idx_e, idx_base))
    dev = np.array(ex.objective_cond_batch(robot, batch, param, idx_e, idx_base, singular_values="device"))
    r = len(idx_base)
    print("objective_cond_batch: host %s device %s" % (host, dev))
    assert np.all(np.abs(dev - host) <= 2 * sc.C_SV * r * 2.0 ** -53 * host ** 2)
    with pytest.raises(ValueError):
        ex.objective_cond_batch(robot, batch, param, idx_e, idx_base, singular_values="lapack")
