"""Synthetic (q, v, a) samples for benchmarks and tests (the role of ``src/figaroh/tools/randomdata.py:20-147`` in the
reference, whose generators need Pinocchio): configurations valid for every joint type of the flattened model --
continuous joints as (cos, sin), a free-flyer as position + unit quaternion -- velocities and accelerations uniform
 -- and ``get_torque_rand`` (randomdata.py:93-147), the torques of such samples."""
import numpy as np


def sample_inputs(model, N, rng, q_range, v_range, a_range):
    q = rng.uniform(-q_range, q_range, (N, model.nq))
    for j in model.joints[1:]:
        if j.jtype == 2:  # continuous: (cos, sin)
            th = rng.uniform(-np.pi, np.pi, N)
            q[:, j.idx_q], q[:, j.idx_q + 1] = np.cos(th), np.sin(th)
        elif j.jtype == 3:  # free-flyer: p in [-1, 1]^3, unit quaternion (x y z w)
            q[:, j.idx_q:j.idx_q + 3] = rng.uniform(-1, 1, (N, 3))
            quat = rng.standard_normal((N, 4))
            q[:, j.idx_q + 3:j.idx_q + 7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    v = rng.uniform(-v_range, v_range, (N, model.nv))
    a = rng.uniform(-a_range, a_range, (N, model.nv))
    return q, v, a


def get_torque_rand(N, robot, q, v, a, param):
    """Joint torques of N samples with the friction, actuator-inertia, offset and coupled-wrist terms (randomdata.py:93-147),
    row j*N + i.  The pin.rnea loop and the three flag blocks are one product W(q, v, a) . phi with phi from
    ``robot.get_standard_parameters(param)`` -- the same fv[j] v + fs[j] sign(v), Ia[j] a, off[j] terms -- in one device
    launch.  The ``has_coupled_wrist`` block is NOT the TX40 coupling columns of the regressor: the reference multiplies Iam6
    by velocities (:126-146); those statements are restated literally on top of the uncoupled launch."""
    from . import regressor
    q, v, a = (np.asarray(x, dtype=np.float64)[:N] for x in (q, v, a))
    nv = robot.model.nv
    p = dict(param, is_joint_torques=True, is_external_wrench=False, device_resident=False)
    phi = np.array(list(robot.get_standard_parameters(p).values()), dtype=np.float64)
    tau = regressor.regressor_times_parameters(robot, q, v, a, p, phi)
    if param["has_coupled_wrist"]:
        s = np.sign(v[:, nv - 2] + v[:, nv - 1])
        tau[(nv - 2) * N:(nv - 1) * N] += (param["Iam6"] * v[:, nv - 1] + param["fvm6"] * v[:, nv - 1] + param["fsm6"] * s)
        tau[(nv - 1) * N:nv * N] += (param["Iam6"] * v[:, nv - 2] + param["fvm6"] * v[:, nv - 2] + param["fsm6"] * s)
    return tau
