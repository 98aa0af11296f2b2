"""Condition-number objective of excitation-trajectory design.

The reference evaluates, thousands of times per Ipopt solve (examples/tiago/optimal_trajectory.py:43-70, 100-133),

    W   = build_regressor_basic(robot, q, v, a, param)
    W_b = build_baseRegressor(build_regressor_reduced(W, idx_e), idx_base)
    W_b = np.vstack((W_stack, W_b))          # optional: regressor of the trajectories found so far
    return np.linalg.cond(W_b)

The singular values of W_b are those of its R factor, and the R factor of a row-stacked matrix is the R factor of the
stacked triangles, so neither W nor W_b is ever stored: one streamed K1 -> TSQR pass over the trajectory samples
(``figh_regressor_tsqr``) gives an r x r triangle, ``figh_tsqr_merge`` folds in the triangle of the previous
trajectories, and the r x r SVD runs on the host or, batched and for r <= 128, on the device (``figh_singular_values_batch``).
:class:`ExcitationProblem` at the end of this module is the optimiser's object on top of it all.
"""
import numpy as np

from .. import _lib
from .._host import host_tail, single_threaded_blas, singular_values_batch, singular_values_batch_device
from . import regressor
from .regressor import _samples_to_device, regressor_flags


def base_columns(ncols, idx_e, idx_base):
    """Columns of W that make up W_b: build_regressor_reduced (np.delete) followed by build_baseRegressor."""
    gone = set(int(i) for i in idx_e)
    kept = [i for i in range(ncols) if i not in gone]
    return np.asarray([kept[int(i)] for i in idx_base], dtype=np.int32)


def base_regressor_triangle(robot, q, v, a, param, idx_e, idx_base, R_stack=None, coupling=False):
    """R factor (r x r, upper) of W_b for the samples (q, v, a), optionally of vstack((W_stack, W_b)) when the
    triangle ``R_stack`` of the previous trajectories is given."""
    mode, flags, ft_mask = regressor_flags(param, coupling)
    dm = robot.device_model()
    _, ncols = dm.shape(mode, flags)
    cols = base_columns(ncols, idx_e, idx_base)
    r = len(cols)
    N, d_q, d_v, d_a = _samples_to_device(robot.model, q, v, a)
    d_idx = _lib.DeviceArray.from_host(cols)
    d_R = _lib.DeviceArray((r * r,), np.float64)
    _lib.regressor_tsqr(dm, mode, flags, ft_mask, N, d_q, d_v, d_a, d_idx, r, None, None, d_R)
    if R_stack is not None:
        R_stack = np.ascontiguousarray(R_stack, dtype=np.float64)
        if R_stack.shape != (r, r):
            raise ValueError("R_stack must be the %d x %d triangle of the previous base regressor" % (r, r))
        pair = np.concatenate([R_stack.reshape(-1), d_R.to_host()])
        d_pair = _lib.DeviceArray.from_host(pair)
        _lib.tsqr_merge(d_pair, 2, r, d_R)
    return np.triu(d_R.to_host().reshape(r, r))


@host_tail
def objective_cond(robot, q, v, a, param, idx_e, idx_base, R_stack=None, coupling=False):
    """np.linalg.cond(W_b) of the reference's ``objective_func`` (2-norm condition number)."""
    R = base_regressor_triangle(robot, q, v, a, param, idx_e, idx_base, R_stack, coupling)
    s = np.linalg.svd(R, compute_uv=False)
    return float(s.max() / s.min())


def _batch_lists(trajectories):
    """[(q_b, v_b, a_b), ...] of equal length -> (B, n_per, q, v, a) with the trajectories back to back, on the host."""
    if len(trajectories) == 0:
        raise ValueError("no trajectory given")
    n_per = len(trajectories[0][0])
    if n_per == 0 or any(len(t[0]) != n_per or len(t[1]) != n_per or len(t[2]) != n_per for t in trajectories):
        raise ValueError("the trajectories of a batch must have the same, non-zero number of samples")
    q = np.concatenate([np.asarray(t[0], dtype=np.float64) for t in trajectories])
    v = np.concatenate([np.asarray(t[1], dtype=np.float64) for t in trajectories])
    a = np.concatenate([np.asarray(t[2], dtype=np.float64) for t in trajectories])
    return len(trajectories), n_per, q, v, a


def _batch_to_device(robot, trajectories):
    """(B, n_per, d_q, d_v, d_a): a :class:`TrajectoryBatch` passes its resident buffers through, a list is concatenated
    and uploaded."""
    if isinstance(trajectories, TrajectoryBatch):
        t = trajectories
        return (t.B, t.n_per) + _samples_to_device(robot.model, t.q, t.v, t.a)[1:]
    B, n_per, q, v, a = _batch_lists(trajectories)
    return (B, n_per) + _samples_to_device(robot.model, q, v, a)[1:]


def base_regressor_triangles_batch(robot, trajectories, param, idx_e, idx_base, R_stack=None, coupling=False):
    """R factors (B x r x r) of the base regressors of B trajectories ``[(q_b, v_b, a_b), ...]`` of equal length, or of a
    :class:`TrajectoryBatch` (resident samples: nothing is concatenated or uploaded).

    Serial chains of 5 to 7 joints in joint-torque mode (UR10), r <= 64, at least 64 samples per trajectory: one launch
    that builds and factors every trajectory's regressor tiles in LDS, W never stored, + one to three merge launches,
    whatever B is (``figh_regressor_tsqr_batch_fused``).  Everything else goes through ``figh_regressor_tsqr_batch``: more
    than 80 base columns (TIAGo, TALOS) in one K1 launch over all samples, one batched TSQR launch and the pair-merge
    levels; up to 80 columns (TX40 with its coupling columns, short trajectories) trajectory by trajectory."""
    d_R, B, r = _base_regressor_triangles_device(robot, trajectories, param, idx_e, idx_base, R_stack, coupling)
    return np.triu(d_R.to_host().reshape(B, r, r))


def _stack_to_device(R_stack, r):
    """The triangle of the previous trajectories as the batched TSQR entries take it, or None."""
    if R_stack is None:
        return None
    R_stack = np.ascontiguousarray(R_stack, dtype=np.float64)
    if R_stack.shape != (r, r):
        raise ValueError("R_stack must be the %d x %d triangle of the previous base regressor" % (r, r))
    return _lib.DeviceArray.from_host(np.triu(R_stack).reshape(-1))


def _triangles_into(dm, mode, flags, ft_mask, B, n_per, d_q, d_v, d_a, d_idx, r, d_stack, d_R):
    """The B triangles of resident samples into ``d_R``: the fused chain launch where it serves, the batched TSQR elsewhere."""
    fused = (mode == _lib.MODE_JOINT_TORQUE and dm.is_chain()
             and _lib.regressor_tsqr_batch_fused(dm, flags, B, n_per, d_q, d_v, d_a, d_idx, r, d_stack, d_R))
    if not fused:  # (ERR_UNSUPPORTED: nothing was launched)
        _lib.regressor_tsqr_batch(dm, mode, flags, ft_mask, B, n_per, d_q, d_v, d_a, d_idx, r, d_stack, d_R)


def _base_regressor_triangles_device(robot, trajectories, param, idx_e, idx_base, R_stack=None, coupling=False):
    """``(d_R, B, r)``: the triangles of :func:`base_regressor_triangles_batch` where the kernels leave them -- B r x r
    matrices back to back whose strict lower part is undefined."""
    if len(trajectories) == 0:
        raise ValueError("no trajectory given")
    mode, flags, ft_mask = regressor_flags(param, coupling)
    dm = robot.device_model()
    _, ncols = dm.shape(mode, flags)
    cols = base_columns(ncols, idx_e, idx_base)
    r = len(cols)
    B, n_per, d_q, d_v, d_a = _batch_to_device(robot, trajectories)
    d_idx = _lib.DeviceArray.from_host(cols)
    d_stack = _stack_to_device(R_stack, r)
    d_R = _lib.DeviceArray((B * r * r,), np.float64)
    _triangles_into(dm, mode, flags, ft_mask, B, n_per, d_q, d_v, d_a, d_idx, r, d_stack, d_R)
    return d_R, B, r


@host_tail
def objective_cond_batch(robot, trajectories, param, idx_e, idx_base, R_stack=None, coupling=False, singular_values="host"):
    """``[np.linalg.cond(W_b) for every trajectory]``: the objective of examples/tiago/optimal_trajectory.py:100-133 at
    the B perturbed trajectories of one finite-difference gradient (numdifftools around ``objective_func``, :296-313),
    r x r SVDs batched on the host.  ``singular_values="device"``: the triangles stay where they are and
    ``figh_singular_values_batch`` (one-sided Jacobi, ``_host.singular_values_batch_device``) sends back B r singular
    values; above 128 base columns that function takes the host route by itself."""
    if singular_values == "device":
        d_R, B, r = _base_regressor_triangles_device(robot, trajectories, param, idx_e, idx_base, R_stack, coupling)
        s = singular_values_batch_device(d_R, B, r)
        return (s.max(axis=1) / s.min(axis=1)).tolist()
    if singular_values != "host":
        raise ValueError("singular_values is 'host' or 'device', got %r" % (singular_values,))
    R = base_regressor_triangles_batch(robot, trajectories, param, idx_e, idx_base, R_stack, coupling)
    s = singular_values_batch(R)
    return (s.max(axis=1) / s.min(axis=1)).tolist()


# ---------------------------------------------------------------------------------------------------------------------
# Effort constraints of the same loop (examples/tiago/utils/cubic_spline.py:448-455, called from
# examples/tiago/optimal_trajectory.py:154 and :288; the constraint Jacobian is taken by finite differences, :321-327, so
# it runs once per perturbed trajectory): pin.rnea per sample, i.e. W . phi without friction / inertia / offset columns.
def _rigid_body_param(param):
    return dict(param, is_joint_torques=True, is_external_wrench=False, has_friction=False, has_actuator_inertia=False,
                has_joint_offset=False, device_resident=False)


def calc_torque(N, robot, q, v, a, param):
    """``tau[j * N + i] = pin.rnea(model, data, q[i], v[i], a[i])[j]`` (cubic_spline.py:448-455) in one device launch."""
    p = _rigid_body_param(param)
    q, v, a = (np.asarray(x, dtype=np.float64)[:N] for x in (q, v, a))
    phi = np.array(list(robot.get_standard_parameters(p).values()), dtype=np.float64)
    return regressor.regressor_times_parameters(robot, q, v, a, p, phi)


def split_batch(tau, B, rows_per_sample, n_per):
    """tau of B trajectories of n_per samples evaluated back to back (row j * B n_per + b n_per + i) -> (B, rows n_per), row
    b in calc_torque's layout (j * n_per + i)."""
    tau = np.asarray(tau).reshape(rows_per_sample, B, n_per)
    return np.ascontiguousarray(tau.transpose(1, 0, 2)).reshape(B, rows_per_sample * n_per)


def calc_torque_batch(robot, trajectories, param):
    """``calc_torque`` of B trajectories ``[(q_b, v_b, a_b), ...]`` of equal length in ONE launch: a (B, nv * n_per) array,
    row b what ``calc_torque(n_per, robot, q_b, v_b, a_b, param)`` returns -- the effort constraints at the B perturbed
    trajectories of one finite-difference Jacobian, next to :func:`objective_cond_batch`.  A :class:`TrajectoryBatch` runs
    the same launch on its resident samples (bit-equal to the list form of the same arrays); with
    ``param["device_resident"]`` its tau stays on the device, a ``DeviceArray`` in the batched layout (row
    j B n_per + b n_per + i) that :func:`constraints_batch` reads."""
    if isinstance(trajectories, TrajectoryBatch):
        t = trajectories
        p = dict(_rigid_body_param(param), device_resident=True)
        phi = np.array(list(robot.get_standard_parameters(p).values()), dtype=np.float64)
        d_tau = regressor.regressor_times_parameters(robot, t.q, t.v, t.a, p, phi)
        return d_tau if param.get("device_resident") else split_batch(d_tau.to_host(), t.B, robot.model.nv, t.n_per)
    B, n_per, q, v, a = _batch_lists(trajectories)
    return split_batch(calc_torque(B * n_per, robot, q, v, a, param), B, robot.model.nv, n_per)


# ---------------------------------------------------------------------------------------------------------------------
# The trajectories of the same loop (examples/tiago/utils/cubic_spline.py:33-233): waypoints -> samples.  The scripts always
# pass velocity and acceleration waypoints, so every ndcurves.exact_cubic of get_active_config has two waypoints and four end
# constraints: the unique quintic through position, velocity and acceleration at both ends.  The functions below state that
# quintic in the operation order of csrc/figh_trajectory.hip (its header comment), one rounded operation per NumPy call, so
# that host mirror and kernel are bit-equal.  Parity with ndcurves is mathematical (the same polynomial), not bitwise.
def spline_times(freq, time_points, n_per=None):
    """(delta_t, T, N, t, k, u) of get_active_config (:133-142): ``t[i] = tps[0] + i * delta_t``, its segment ``k[i]`` (the
    largest k with ``tps[k] <= t[i]``, at most n_wps - 2) and local time ``u[i] = min(t[i] - tps[k], tps[k+1] - tps[k])``.
    ``n_per``: that many samples instead of the reference's N, as ``figh_spline_sample`` takes it -- a prefix below N; above it
    the samples behind the last time point sit at the end of the last segment."""
    tps = np.asarray(time_points, dtype=np.float64).reshape(-1)
    if len(tps) < 2 or not np.all(tps[1:] > tps[:-1]) or not np.isfinite(tps[[0, -1]]).all():
        raise ValueError("time points must be finite and strictly increasing")
    delta_t = 1 / freq
    T = tps[-1] - tps[0]
    N = int(T / delta_t) + 1
    t = tps[0] + np.arange(N if n_per is None else n_per, dtype=np.float64) * delta_t
    k = np.minimum(np.searchsorted(tps, t, side="right") - 1, len(tps) - 2)
    u = np.minimum(t - tps[k], tps[k + 1] - tps[k])
    return delta_t, T, N, t, k, u


def spline_coefficients(time_points, wps, vel_wps, acc_wps):
    """c0 .. c5 of every segment: ``wps`` is (..., n_act, n_wps), the result (..., n_act, n_wps - 1, 6)."""
    tps = np.asarray(time_points, dtype=np.float64).reshape(-1)
    wps, vel, acc = (np.asarray(x, dtype=np.float64) for x in (wps, vel_wps, acc_wps))
    h = tps[1:] - tps[:-1]
    h2 = h * h
    h3 = h2 * h
    h4 = h3 * h
    h5 = h4 * h
    p0, p1 = wps[..., :-1], wps[..., 1:]
    v0, v1 = vel[..., :-1], vel[..., 1:]
    a0, a1 = acc[..., :-1], acc[..., 1:]
    D = p1 - p0
    c3 = ((20.0 * D - (8.0 * v1 + 12.0 * v0) * h) - (3.0 * a0 - a1) * h2) / (2.0 * h3)
    c4 = ((-30.0 * D + (14.0 * v1 + 16.0 * v0) * h) + (3.0 * a0 - 2.0 * a1) * h2) / (2.0 * h4)
    c5 = ((12.0 * D - (6.0 * (v1 + v0)) * h) - (a0 - a1) * h2) / (2.0 * h5)
    return np.stack(np.broadcast_arrays(p0, v0, a0 / 2.0, c3, c4, c5), axis=-1)


def spline_samples(coef, k, u):
    """(q, dq, ddq), each (..., N, n_act), of the segments ``coef`` (..., n_act, n_seg, 6) at the samples (k, u)."""
    c = np.moveaxis(coef[..., k, :], -3, -2)  # (..., N, n_act, 6)
    u = u[:, None]
    c0, c1, c2, c3, c4, c5 = (c[..., m] for m in range(6))
    q = ((((c5 * u + c4) * u + c3) * u + c2) * u + c1) * u + c0
    dq = ((((5.0 * c5) * u + 4.0 * c4) * u + 3.0 * c3) * u + 2.0 * c2) * u + c1
    ddq = (((20.0 * c5) * u + 12.0 * c4) * u + 6.0 * c3) * u + 2.0 * c2
    return q, dq, ddq


class CubicSpline:
    """``CubicSpline`` of examples/tiago/utils/cubic_spline.py:33-233: the same constructor, attributes, ``get_active_config``
    / ``get_full_config`` / ``check_cfg_constraints``.  Host arrays in, host arrays out through the NumPy mirror above;
    ``get_full_config(..., device_resident=True)`` returns three ``GpuMatrix`` written by ``figh_spline_sample``.  The time of
    a sample is capped at the end of its segment: where rounding puts the last sample behind the last time point ndcurves
    raises, this class evaluates the end of the last segment.  Plotting and waypoint pools are not mirrored; the self-collision
    distances of the constraint vector come from ``tools.robotcollisions`` (:func:`constraint_vector`,
    :func:`constraints_batch` and :func:`evaluate_waypoints_batch` with ``collision=``)."""

    def __init__(self, robot, num_waypoints, active_joints, soft_lim=0):
        self.robot = robot
        self.rmodel = robot.model
        self.num_waypoints = num_waypoints
        self.act_Jid = [self.rmodel.getJointId(i) for i in active_joints]
        self.act_Jname = [self.rmodel.names[jid] for jid in self.act_Jid]
        self.act_J = [self.rmodel.joints[jid] for jid in self.act_Jid]
        self.act_idxq = [J.idx_q for J in self.act_J]
        self.act_idxv = [J.idx_v for J in self.act_J]
        self.dim_q = (len(self.act_idxq), self.num_waypoints)
        self.dim_v = (len(self.act_idxv), self.num_waypoints)
        m = self.rmodel
        self.upper_q = m.upperPositionLimit[self.act_idxq]
        self.lower_q = m.lowerPositionLimit[self.act_idxq]
        self.upper_dq = m.velocityLimit[self.act_idxv]
        self.lower_dq = -m.velocityLimit[self.act_idxv]
        self.upper_effort = m.effortLimit[self.act_idxv]
        self.lower_effort = -m.effortLimit[self.act_idxv]
        if soft_lim > 0:  # (:64-80: each lower limit is moved by the range that is left after its upper limit moved)
            self.upper_q = self.upper_q - soft_lim * abs(self.upper_q - self.lower_q)
            self.lower_q = self.lower_q + soft_lim * abs(self.upper_q - self.lower_q)
            self.upper_dq = self.upper_dq - soft_lim * abs(self.upper_dq - self.lower_dq)
            self.lower_dq = self.lower_dq + soft_lim * abs(self.upper_dq - self.lower_dq)
            self.upper_effort = self.upper_effort - soft_lim * abs(self.upper_effort - self.lower_effort)
            self.lower_effort = self.lower_effort + soft_lim * abs(self.upper_effort - self.lower_effort)

    def _check(self, waypoints, vel_waypoints, acc_waypoints):
        pad = " " * 40  # (the reference's messages are string literals continued over a line break)
        assert self.dim_q == waypoints.shape, "(Pos) Check size " + pad + "(num_active_joints,num_waypoints)!"
        if vel_waypoints is None or acc_waypoints is None:
            raise NotImplementedError(
                "without velocity and acceleration waypoints the reference builds ndcurves' unconstrained exact_cubic, whose "
                "polynomial is not restated here (ndcurves is not a dependency); pass both, zero arrays included, as the "
                "scripts do")
        assert self.dim_v == vel_waypoints.shape, "(Vel) Check size" + pad + "(num_active_joints, num_waypoints)!"
        assert self.dim_v == acc_waypoints.shape, "(Acc) Check size" + pad + "(num_active_joints, num_waypoints)!"
        for J, name in zip(self.act_J, self.act_Jname):
            if J.nq != 1 or J.nv != 1:
                raise ValueError("active joint %s is not one revolute or prismatic degree of freedom (nq = %d, nv = %d): a "
                                 "continuous or free-flyer joint has no waypoint in joint coordinates" % (name, J.nq, J.nv))

    def get_active_config(self, freq, time_points, waypoints, vel_waypoints=None, acc_waypoints=None):
        """(t, p_act, v_act, a_act): the splines of the active joints, ``t`` an (N, 1) column (:82-156)."""
        self._check(waypoints, vel_waypoints, acc_waypoints)
        self.delta_t, self.T, self.N, t, k, u = spline_times(freq, time_points)
        if np.size(time_points) != self.num_waypoints:
            raise ValueError("%d time points for %d waypoints" % (np.size(time_points), self.num_waypoints))
        coef = spline_coefficients(time_points, waypoints, vel_waypoints, acc_waypoints)
        self.t = t.reshape(-1, 1)
        self.q_act, self.dq_act, self.ddq_act = spline_samples(coef, k, u)
        return self.t, self.q_act, self.dq_act, self.ddq_act

    def get_full_config(self, freq, time_points, waypoints, vel_waypoints=None, acc_waypoints=None, device_resident=False):
        """(t, p_full, v_full, a_full): the active joints' profiles in full configurations, ``robot.q0`` and zeros in the
        other columns (:158-181).  ``device_resident``: p, v, a as ``GpuMatrix`` from ``figh_spline_sample``."""
        if device_resident:
            self._check(waypoints, vel_waypoints, acc_waypoints)
            batch = spline_batch(self, freq, time_points, np.asarray(waypoints)[None], vel_waypoints, acc_waypoints)
            self.delta_t, self.T, self.N, self.t = batch.delta_t, batch.T, batch.n_per, batch.t
            return batch.t, batch.q, batch.v, batch.a
        t, p_act, v_act, a_act = self.get_active_config(freq, time_points, waypoints, vel_waypoints, acc_waypoints)
        self.q_full = np.array([self.robot.q0] * self.N)
        self.dq_full = np.array([np.zeros_like(self.robot.v0)] * self.N)
        self.ddq_full = np.array([np.zeros_like(self.robot.v0)] * self.N)
        self.q_full[:, self.act_idxq] = p_act
        self.dq_full[:, self.act_idxv] = v_act
        self.ddq_full[:, self.act_idxv] = a_act
        return t, self.q_full, self.dq_full, self.ddq_full

    def check_cfg_constraints(self, q, v=None, tau=None, soft_lim=0):
        """True when a position, velocity or effort limit of an active joint is violated at some sample (:183-233); prints
        what the reference prints."""
        m = self.rmodel
        violated = False
        for i in range(q.shape[0]):
            for j in self.act_idxq:
                delta_lim = soft_lim * abs(m.upperPositionLimit[j] - m.lowerPositionLimit[j])
                if q[i, j] > m.upperPositionLimit[j] - delta_lim:
                    print("Joint q %d upper limit violated!" % j)
                    violated = True
                elif q[i, j] < m.lowerPositionLimit[j] + delta_lim:
                    print("Joint position idx_q %d lower limit violated!" % j)
                    violated = True
        for x, limit, text in ((v, m.velocityLimit, "Joint vel idx_v %d limits violated!"),
                               (tau, m.effortLimit, "Joint effort idx_v %d limits violated!")):
            if x is None:
                continue
            for i in range(x.shape[0]):
                for j in self.act_idxv:
                    if abs(x[i, j]) > (1 - soft_lim) * abs(limit[j]):
                        print(text % j)
                        violated = True
        if not violated:
            print("SUCCEEDED to generate waypoints for  a feasible initial cubic spline")
        else:
            print("FAILED to generate a feasible cubic spline")
        return violated


class TrajectoryBatch:
    """B trajectories of n_per samples, resident: ``q`` (B n_per x nq), ``v``, ``a`` (B n_per x nv) as ``GpuMatrix`` with the
    trajectories back to back -- what :func:`base_regressor_triangles_batch`, :func:`objective_cond_batch` and
    :func:`calc_torque_batch` take in place of a list -- and the (n_per, 1) time column ``t`` they share."""

    def __init__(self, B, n_per, q, v, a, t, delta_t=None, T=None):
        self.B, self.n_per, self.q, self.v, self.a, self.t = int(B), int(n_per), q, v, a, t
        self.delta_t, self.T = delta_t, T

    def __len__(self):
        return self.B

    def numpy(self):
        """``[(q_b, v_b, a_b), ...]`` on the host: the list form of the same arrays."""
        q, v, a = (x.numpy().reshape(self.B, self.n_per, -1) for x in (self.q, self.v, self.a))
        return [(q[b], v[b], a[b]) for b in range(self.B)]


def waypoints_from_search_variables(X_batch, wp_init, n_wps, n_act):
    """(B, n_act, n_wps) waypoint arrays from B rows of the optimiser's search variables: per row the ``reshape -> vstack ->
    transpose`` of examples/tiago/optimal_trajectory.py:116-119."""
    X = np.asarray(X_batch, dtype=np.float64)
    X = X.reshape(-1, n_wps - 1, n_act)
    first = np.broadcast_to(np.asarray(wp_init, dtype=np.float64).reshape(1, 1, n_act), (X.shape[0], 1, n_act))
    return np.ascontiguousarray(np.concatenate((first, X), axis=1).transpose(0, 2, 1))


def spline_batch(spline, freq, tps, wps_batch, vel_wps, acc_wps):
    """B waypoint sets ``wps_batch`` (B, n_act, n_wps) -> :class:`TrajectoryBatch` in two launches (``figh_spline_sample``).
    ``vel_wps`` / ``acc_wps``: (n_act, n_wps), one set for all trajectories as in the script, or (B, n_act, n_wps).  What
    crosses the bus is the waypoints: B n_act n_wps doubles."""
    from ..device import GpuMatrix
    wps = np.ascontiguousarray(wps_batch, dtype=np.float64)
    n_act, n_wps = spline.dim_q
    if wps.ndim != 3 or wps.shape[1:] != (n_act, n_wps):
        raise ValueError("wps_batch must be (B, %d, %d), got %r" % (n_act, n_wps, wps.shape))
    B = wps.shape[0]
    if vel_wps is None or acc_wps is None:
        spline._check(wps[0], None, None)
    strides, bufs, first = [], [], []
    for x in (vel_wps, acc_wps):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape not in ((n_act, n_wps), (B, n_act, n_wps)):
            raise ValueError("velocity / acceleration waypoints must be (%d, %d) or (%d, %d, %d), got %r"
                             % (n_act, n_wps, B, n_act, n_wps, x.shape))
        strides.append(0 if x.ndim == 2 else n_act * n_wps)
        first.append(x if x.ndim == 2 else x[0])
        bufs.append(x.reshape(-1))
    spline._check(wps[0], first[0], first[1])
    delta_t, T, n_per, t, _, _ = spline_times(freq, tps)
    if np.size(tps) != n_wps:
        raise ValueError("%d time points for %d waypoints" % (np.size(tps), n_wps))
    m = spline.rmodel
    q, v, a = (GpuMatrix.empty(B * n_per, w) for w in (m.nq, m.nv, m.nv))
    bufs = [_lib.DeviceArray.from_host(x) for x in bufs]
    d_wps = _lib.DeviceArray.from_host(wps.reshape(-1))
    d_q0 = _lib.DeviceArray.from_host(np.ascontiguousarray(spline.robot.q0, dtype=np.float64))
    _lib.spline_sample(spline.robot.device_model(), B, n_wps, n_per, freq, spline.act_idxq, spline.act_idxv,
                       np.asarray(tps, dtype=np.float64).reshape(-1), d_wps, bufs[0], strides[0], bufs[1], strides[1], d_q0,
                       q.ptr, q.ld, v.ptr, a.ptr, v.ld)
    return TrajectoryBatch(B, n_per, q, v, a, t.reshape(-1, 1), delta_t, T)


def waypoint_sample_indices(t, tps):
    """idx_waypoints of get_constraints_all_samples (:157-162): the samples whose time EQUALS one of ``tps[1:]``."""
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    return np.flatnonzero(np.isin(t, np.asarray(tps, dtype=np.float64).reshape(-1)[1:]))


def constraint_vector(spline, t_f, p_f, v_f, tau, tps, collision=None):
    """get_constraints_all_samples (examples/tiago/optimal_trajectory.py:156-188) of one trajectory on host arrays: positions
    of the active joints at the waypoints, their velocities and efforts at every sample and, with a ``CollisionWrapper`` as
    ``collision``, the distances of its pairs at the waypoint samples (waypoint-major, pair-minor: the reference's np.append
    over idx_waypoints of getDistances(), :176-182), concatenated.  ``collision=None``: the first three parts."""
    Ns = len(p_f)
    idx = waypoint_sample_indices(t_f, tps)
    q_c = np.asarray(p_f)[idx, :][:, spline.act_idxq]
    v_c = np.asarray(v_f)[:, spline.act_idxv]
    tau = np.asarray(tau)
    tau_c = np.zeros((Ns, len(spline.act_idxv)))
    for k, j in enumerate(spline.act_idxv):
        tau_c[:, k] = tau[j * Ns:(j + 1) * Ns]
    if collision is None:
        return np.concatenate((q_c, v_c, tau_c), axis=None)
    dist_all = np.zeros(0)
    if len(idx):
        collision.computeCollisions(np.asarray(p_f)[idx, :])
        dist_all = collision.getDistances().reshape(-1)
    return np.concatenate((q_c, v_c, tau_c, dist_all), axis=None)


def collision_distances_batch(robot, batch, idx, geom_model=None, device_resident=False, tol=None, max_iter=None):
    """(B, n_idx n_pairs): the self-collision distances of every trajectory of a :class:`TrajectoryBatch` at its samples
    ``idx`` (None: every sample), waypoint-major and pair-minor per trajectory -- the reference's np.append over
    idx_waypoints of getDistances() (examples/tiago/optimal_trajectory.py:176-182) -- in one ``figh_collision_distances``
    launch on the resident configurations.  ``device_resident``: the result stays on the device, a ``GpuMatrix``."""
    from ..device import GpuMatrix
    from . import robotcollisions as rc
    gm = robot.geom_model if geom_model is None else geom_model
    n_pairs = len(gm.collisionPairs)
    n_idx = batch.n_per if idx is None else len(idx)
    out = GpuMatrix.empty(batch.B, n_idx * n_pairs)
    if n_idx * n_pairs:
        rc.collision_distances_device(robot, gm, batch.q.ptr, batch.q.ld, batch.B, batch.n_per, idx, out.ptr, out.ld,
                                      rc.DEFAULT_TOL if tol is None else tol,
                                      rc.DEFAULT_MAX_ITER if max_iter is None else max_iter)
    return out if device_resident else out.buf.to_host().reshape(batch.B, n_idx * n_pairs)


def constraint_bounds(spline, n_wps, Ns, n_pairs=0, margin=0.01):
    """``(cl, cu)`` of get_constr_value (examples/tiago/optimal_trajectory.py:202-243) as lists: the position limits of the
    active joints per waypoint behind the first, their velocity and effort limits per sample, and ``margin`` (1 cm) and 2e19
    ("no limit") for the ``n_pairs`` collision distances of each of those waypoints."""
    cl, cu = [], []
    for lower, upper, reps in ((spline.lower_q, spline.upper_q, n_wps - 1), (spline.lower_dq, spline.upper_dq, Ns),
                               (spline.lower_effort, spline.upper_effort, Ns)):
        for _ in range(reps):
            cl.extend(lower)
            cu.extend(upper)
    cl += [margin] * n_pairs * (n_wps - 1)
    cu += [2 * 1e19] * n_pairs * (n_wps - 1)
    return cl, cu


def constraints_batch(spline, batch, tau, tps, collision=None):
    """(B, n_con) host array, row b = :func:`constraint_vector` of trajectory b, gathered on the device
    (``figh_excitation_constraints``) and brought back in one copy.  ``tau``: what ``calc_torque_batch(robot, batch,
    dict(param, device_resident=True))`` returns (the batched layout).  With a ``CollisionWrapper`` as ``collision`` the rows
    are (n_wps - 1) n_pairs longer: ``figh_collision_distances`` writes the distances at the waypoint samples straight into
    the tail of the rows of the same buffer -- one output buffer, one download."""
    if not isinstance(tau, _lib.DeviceArray):
        tau = _lib.DeviceArray.from_host(np.ascontiguousarray(tau, dtype=np.float64).reshape(-1))
    nv = spline.rmodel.nv
    if tau.size != nv * batch.B * batch.n_per:
        raise ValueError("tau has %d entries, the batch has %d x %d samples of %d efforts" % (tau.size, batch.B, batch.n_per, nv))
    idx = waypoint_sample_indices(batch.t, tps)
    n_act = len(spline.act_idxv)
    n_con = len(idx) * n_act + 2 * batch.n_per * n_act
    if collision is None:
        out = _lib.DeviceArray((batch.B * n_con,), np.float64)
        _lib.excitation_constraints(spline.robot.device_model(), batch.B, batch.n_per, spline.act_idxq, spline.act_idxv, idx,
                                    batch.q.ptr, batch.q.ld, batch.v.ptr, batch.v.ld, tau, out.ptr, n_con)
        return out.to_host().reshape(batch.B, n_con)
    from . import robotcollisions as rc
    n_dist = len(idx) * len(collision.gmodel.collisionPairs)
    ld = n_con + n_dist
    out = _lib.DeviceArray((batch.B * ld,), np.float64)
    _lib.excitation_constraints(spline.robot.device_model(), batch.B, batch.n_per, spline.act_idxq, spline.act_idxv, idx,
                                batch.q.ptr, batch.q.ld, batch.v.ptr, batch.v.ld, tau, out.ptr, ld)
    if n_dist:
        rc.collision_distances_device(spline.robot, collision.gmodel, batch.q.ptr, batch.q.ld, batch.B, batch.n_per, idx,
                                      out.ptr + 8 * n_con, ld, collision.tol, collision.max_iter)
    return out.to_host().reshape(batch.B, ld)


def evaluate_waypoints_batch(robot, spline, freq, tps, X_batch, vel_wps, acc_wps, wp_init, param, idx_e, idx_base,
                             R_stack=None, collision=None):
    """``(conds, constraints)``: ``objective`` and ``constraints`` of the script's Ipopt problem
    (examples/tiago/optimal_trajectory.py:100-188, :296-327) at the B rows of ``X_batch`` -- the points of one finite-difference
    gradient or Jacobian.  Waypoints go up, B condition numbers (through B r x r triangles) and the (B, n_con) constraint
    vectors come back; the samples, v and tau never leave the device.  ``collision``: a ``CollisionWrapper`` whose pairs'
    distances at the waypoint samples are the fourth part of every constraint vector (:func:`constraints_batch`); None: the
    first three parts."""
    n_act, n_wps = spline.dim_q
    wps = waypoints_from_search_variables(X_batch, wp_init, n_wps, n_act)
    batch = spline_batch(spline, freq, tps, wps, vel_wps, acc_wps)
    conds = objective_cond_batch(robot, batch, param, idx_e, idx_base, R_stack)
    d_tau = calc_torque_batch(robot, batch, dict(param, device_resident=True))
    if collision is None:
        return conds, constraints_batch(spline, batch, d_tau, tps)
    return conds, constraints_batch(spline, batch, d_tau, tps, collision)


# ---------------------------------------------------------------------------------------------------------------------
# The Ipopt problem of the same script (Problem_cond_Wb, examples/tiago/optimal_trajectory.py:246-330): objective, gradient,
# constraints and jacobian of one X from ONE pass over the finite-difference stencil.
SCHEMES = {"2-point": 2, "3-point": 3}


def finite_difference_steps(x, scheme="2-point", rel_step=None):
    """``(h, dx)`` of SciPy's rules (scipy.optimize._numdiff without bounds): h = rel_step sign(x) max(1, |x|), sign(0) = 1,
    rel_step = sqrt(eps) for the 2-point and eps^(1/3) for the 3-point scheme; ``dx`` is the step as the arithmetic took
    it, (x + h) - x or (x + h) - (x - h) -- what ``calibration_tools.fkm_jacobian_2point`` divides by as well."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if scheme not in SCHEMES:
        raise ValueError("scheme is '2-point' or '3-point', got %r" % (scheme,))
    eps = np.finfo(np.float64).eps
    if rel_step is None:
        rel_step = eps ** 0.5 if scheme == "2-point" else eps ** (1 / 3)
    h = rel_step * ((x >= 0).astype(np.float64) * 2 - 1) * np.maximum(1.0, np.abs(x))
    dx = (x + h) - x if scheme == "2-point" else (x + h) - (x - h)
    return h, dx


def finite_difference_stencil(x, h, scheme="2-point"):
    """The rows at which one finite-difference gradient evaluates: row 0 is x, row 1 + j is x + h_j e_j and, for the 3-point
    scheme, row 1 + n + j is x - h_j e_j -- the row order of ``figh_difference_quotients``."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = len(x)
    sign = np.concatenate((np.zeros((1, n)), np.eye(n)) + ((-np.eye(n),) if scheme == "3-point" else ()))
    return np.where(sign == 0, x, x + sign * h)


def difference_quotients(C, dx, scheme="2-point"):
    """NumPy statement of ``figh_difference_quotients``: the (n_con, n_var) array ``(C[1 + j] - C[0]) / dx[j]`` (2-point) or
    ``(C[1 + j] - C[1 + n_var + j]) / dx[j]`` (3-point) from the rows of :func:`finite_difference_stencil`."""
    C, dx = np.asarray(C, dtype=np.float64), np.asarray(dx, dtype=np.float64).reshape(-1)
    n = len(dx)
    C = C.reshape(C.shape[0], -1)
    if C.shape[0] != (1 + n if SCHEMES[scheme] == 2 else 1 + 2 * n):
        raise ValueError("%d rows for %d variables and the %s scheme" % (C.shape[0], n, scheme))
    lo = C[0] if SCHEMES[scheme] == 2 else C[1 + n:]
    return np.ascontiguousarray(((C[1:1 + n] - lo) / dx[:, None]).T)


class ExcitationProblem:
    """``Problem_cond_Wb`` of examples/tiago/optimal_trajectory.py:246-330 -- ``objective(X)``, ``gradient(X)``,
    ``constraints(X)``, ``jacobian(X)``, ``hessian(...) -> False`` -- with the finite differences of the reference (nd.Gradient
    / nd.Jacobian around the objective and the constraints, :308-327) taken over ONE device pass: the stencil of
    :func:`finite_difference_stencil` goes up as waypoints (B = n_var + 1 or 2 n_var + 1 rows), the B trajectories are sampled,
    factored and constrained on the device, and what comes back is B r singular values with their status, the (n_con, n_var)
    Jacobian (``figh_difference_quotients``) and row 0 of the constraints; neither the B x n_con rows nor the B triangles cross
    the bus.  ``bounds()`` is get_bounds (:191-199), ``constraint_bounds()`` get_constr_value (:202-243).

    Ipopt calls all four methods at one X: a *derivative pass* (the whole stencil) serves the four, a *value pass* (B = 1)
    serves objective and constraints at a line-search point; both are cached on the bytes of X.  An X that no cached pass
    holds costs a value pass when objective or constraints ask first and a derivative pass when gradient or jacobian do;
    the very first evaluation of the object is a derivative pass whoever asks (an optimiser starts at an iterate, not at a
    trial point).  What does not change during
    a run stays on the device across calls: q0, the velocity and acceleration waypoints, the base-column list, R_stack and the
    standard parameters.  The time points, the active-joint and waypoint-sample index lists and the collision geometry table
    are host arguments of their entries and go with every call.

    Steps are SciPy's (:func:`finite_difference_steps`); numdifftools' Richardson extrapolation is not mirrored.

    Noise.  A finite-difference gradient of cond(W_b) is as good as the condition numbers are reproducible.  On either route
    (``singular_values="device"``: one-sided Jacobi on the resident triangles; ``"host"``: LAPACK on the downloaded ones)
    sigma_min carries a relative error of the order r 2^-53 cond, and the triangles themselves are reproduced only to
    rounding on the fused chain path, so a quotient with step h has noise of the order r 2^-53 cond^2 / h: 3e-3 per
    gradient entry at r = 40, cond = 100 and h = 1.5e-8.  Hence ``rel_step`` is a parameter, and the 3-point scheme's larger
    default step (6e-6) is the quieter one.  The device route falls back to the host per matrix where the kernel did not converge
    (``last_pass.host_fallbacks``)."""

    def __init__(self, robot, spline, freq, tps, vel_wps, acc_wps, wp_init, param, idx_e, idx_base, R_stack=None,
                 collision=None, scheme="2-point", rel_step=None, singular_values="device"):
        if scheme not in SCHEMES:
            raise ValueError("scheme is '2-point' or '3-point', got %r" % (scheme,))
        if singular_values not in ("device", "host"):
            raise ValueError("singular_values is 'host' or 'device', got %r" % (singular_values,))
        self.robot, self.spline, self.freq, self.collision = robot, spline, freq, collision
        self.scheme, self.rel_step, self.singular_values = scheme, rel_step, singular_values
        self.tps = np.asarray(tps, dtype=np.float64).reshape(-1)
        self.n_act, self.n_wps = spline.dim_q
        if len(self.tps) != self.n_wps:
            raise ValueError("%d time points for %d waypoints" % (len(self.tps), self.n_wps))
        self.n_var = (self.n_wps - 1) * self.n_act
        self.wp_init = np.asarray(wp_init, dtype=np.float64).reshape(-1)
        vel, acc = (np.ascontiguousarray(x, dtype=np.float64) for x in (vel_wps, acc_wps))
        if vel.shape != spline.dim_v or acc.shape != spline.dim_v:
            raise ValueError("velocity / acceleration waypoints must be (%d, %d)" % spline.dim_v)
        spline._check(np.zeros(spline.dim_q), vel, acc)
        self.delta_t, self.T, self.n_per, t, _, _ = spline_times(freq, self.tps)
        self.t = t.reshape(-1, 1)
        self.idx_waypoints = waypoint_sample_indices(t, self.tps)
        self.n_pairs = 0 if collision is None else len(collision.gmodel.collisionPairs)
        self.n_dist = len(self.idx_waypoints) * self.n_pairs
        self.n_con = len(self.idx_waypoints) * self.n_act + 2 * self.n_per * self.n_act + self.n_dist
        # the two regressor calls of a pass: the base regressor's triangle, and rnea as W . phi of the rigid-body columns
        self._dm = robot.device_model()
        self._tri = regressor_flags(param, False)
        _, ncols = self._dm.shape(*self._tri[:2])
        cols = base_columns(ncols, idx_e, idx_base)
        self.r = len(cols)
        self._rigid = _rigid_body_param(param)
        self._tau = regressor_flags(self._rigid, False)
        _, ncols_tau = self._dm.shape(*self._tau[:2])
        self._phi = np.array(list(robot.get_standard_parameters(self._rigid).values()), dtype=np.float64)
        # resident across calls
        self._d_idx = _lib.DeviceArray.from_host(cols)
        self._d_stack = _stack_to_device(R_stack, self.r)
        self._d_vel, self._d_acc = _lib.DeviceArray.from_host(vel.reshape(-1)), _lib.DeviceArray.from_host(acc.reshape(-1))
        self._d_q0 = _lib.DeviceArray.from_host(np.ascontiguousarray(robot.q0, dtype=np.float64))
        self._d_phi = _lib.DeviceArray.from_host(regressor.expand_parameters(self._phi, ncols_tau))
        self._buffers = {}  # B -> the pass buffers (two sizes in a run: 1 and the stencil)
        self._value = self._derivative = None  # (bytes of X, pass result)
        self.last_pass = None
        self.value_passes = self.derivative_passes = 0

    # ------------------------------------------------------------------------------------------------ the reference's methods
    def objective(self, X):
        return float(self._values_at(X).conds[0])

    def constraints(self, X):
        return self._values_at(X).c0

    def gradient(self, X):
        p = self._derivatives_at(X)
        n = self.n_var
        lo = p.conds[0] if self.scheme == "2-point" else p.conds[1 + n:]
        return (p.conds[1:1 + n] - lo) / p.dx

    def jacobian(self, X):
        return self._derivatives_at(X).jacobian

    def hessian(self, X=None, lagrange=None, obj_factor=None):
        return False

    def bounds(self):
        """``(lb, ub)`` of get_bounds (:191-199): the position limits of the active joints per waypoint behind the first."""
        lb, ub = [], []
        for _ in range(1, self.n_wps):
            lb.extend(self.spline.lower_q)
            ub.extend(self.spline.upper_q)
        return lb, ub

    def constraint_bounds(self, margin=0.01):
        return constraint_bounds(self.spline, self.n_wps, self.n_per, self.n_pairs, margin)

    # ------------------------------------------------------------------------------------------------------------ the passes
    def _key(self, X):
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1)
        if X.size != self.n_var:
            raise ValueError("X has %d entries, the problem %d search variables" % (X.size, self.n_var))
        return X.tobytes()

    def _values_at(self, X):
        key = self._key(X)
        for cached in (self._derivative, self._value):
            if cached is not None and cached[0] == key:
                return cached[1]
        if self._derivative is None:  # the first point of a run is an iterate, whose derivatives are asked for next
            return self._derivatives_at(X)
        self._value = (key, self._pass(np.frombuffer(key, dtype=np.float64).reshape(1, -1), None))
        self.value_passes += 1
        return self._value[1]

    def _derivatives_at(self, X):
        key = self._key(X)
        if self._derivative is None or self._derivative[0] != key:
            x = np.frombuffer(key, dtype=np.float64)
            h, dx = finite_difference_steps(x, self.scheme, self.rel_step)
            self._derivative = (key, self._pass(finite_difference_stencil(x, h, self.scheme), dx))
            self.derivative_passes += 1
        return self._derivative[1]

    def _pass_buffers(self, B):
        from ..device import GpuMatrix
        if B not in self._buffers:
            m = self.spline.rmodel
            q, v, a = (GpuMatrix.empty(B * self.n_per, w) for w in (m.nq, m.nv, m.nv))
            self._buffers[B] = (q, v, a, _lib.DeviceArray((B * self.r * self.r,), np.float64),
                                _lib.DeviceArray((m.nv * B * self.n_per,), np.float64),
                                _lib.DeviceArray((B * self.n_con,), np.float64),
                                _lib.DeviceArray((self.n_con * self.n_var,), np.float64) if B > 1 else None,
                                _lib.DeviceArray((self.n_con,), np.float64) if B > 1 else None)
        return self._buffers[B]

    def _pass(self, Xs, dx):
        """One pass over the rows ``Xs`` (B, n_var); ``dx`` None: a value pass."""
        from types import SimpleNamespace
        B = Xs.shape[0]
        sp, dm, n_per, r, n_con = self.spline, self._dm, self.n_per, self.r, self.n_con
        q, v, a, d_R, d_tau, d_C, d_J, d_c0 = self._pass_buffers(B)
        d_wps = _lib.DeviceArray.from_host(waypoints_from_search_variables(Xs, self.wp_init, self.n_wps, self.n_act).reshape(-1))
        _lib.spline_sample(dm, B, self.n_wps, n_per, self.freq, sp.act_idxq, sp.act_idxv, self.tps, d_wps, self._d_vel, 0,
                           self._d_acc, 0, self._d_q0, q.ptr, q.ld, v.ptr, a.ptr, v.ld)
        mode, flags, ft_mask = self._tri
        _triangles_into(dm, mode, flags, ft_mask, B, n_per, q.buf, v.buf, a.buf, self._d_idx, r, self._d_stack, d_R)
        if self.singular_values == "device":
            s, sweeps, fallbacks = singular_values_batch_device(d_R, B, r, return_status=True)
        else:
            with single_threaded_blas():
                s, sweeps, fallbacks = singular_values_batch(np.triu(d_R.to_host().reshape(B, r, r))), None, 0
        conds = s.max(axis=1) / s.min(axis=1)
        mode, flags, ft_mask = self._tau
        if not _lib.regressor_apply(dm, mode, flags, ft_mask, B * n_per, q.buf, v.buf, a.buf, self._d_phi, d_tau):
            d_tau = regressor.regressor_times_parameters_device(self.robot, q.buf, v.buf, a.buf, B * n_per, self._rigid, self._phi)
        _lib.excitation_constraints(dm, B, n_per, sp.act_idxq, sp.act_idxv, self.idx_waypoints, q.ptr, q.ld, v.ptr, v.ld, d_tau,
                                    d_C.ptr, n_con)
        if self.n_dist:
            from . import robotcollisions as rc
            rc.collision_distances_device(self.robot, self.collision.gmodel, q.ptr, q.ld, B, n_per, self.idx_waypoints,
                                          d_C.ptr + 8 * (n_con - self.n_dist), n_con, self.collision.tol, self.collision.max_iter)
        if dx is None:
            c0, jac = d_C.to_host(), None
        else:
            d_dx = _lib.DeviceArray.from_host(dx)
            _lib.difference_quotients(d_C, n_con, n_con, self.n_var, SCHEMES[self.scheme], d_dx, d_J, self.n_var)
            _lib.check(_lib.load().figh_memcpy_d2d(d_c0.ptr, d_C.ptr, 8 * n_con))  # row 0 alone comes down
            c0, jac = d_c0.to_host(), d_J.to_host().reshape(n_con, self.n_var)
        self.last_pass = SimpleNamespace(B=B, conds=conds, dx=dx, sweeps=sweeps, host_fallbacks=fallbacks, sigma=s, c0=c0,
                                         jacobian=jac)
        return self.last_pass
