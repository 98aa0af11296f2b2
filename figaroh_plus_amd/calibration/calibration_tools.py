"""Geometric calibration on the package's kernels: the kinematic regressor, the updated forward kinematics of the
Levenberg-Marquardt cost, and the base-parameter reduction of ``src/figaroh/calibration/calibration_tools.py``.

* ``calculate_kinematics_model`` (``:1368-1392``), ``get_sup_joints`` / ``get_rel_transform`` / ``get_rel_kinreg`` /
  ``get_rel_jac`` (``:592-740``) and ``calculate_identifiable_kinematics_model`` (``:1395-1466``): Pinocchio's
  ``computeFrameKinematicRegressor(..., LOCAL)`` and ``computeFrameJacobian(..., LOCAL)`` restated on the flat model
  (conventions of SURVEY.md A.1, written out in ``kinematic_regressor_batch``) -- float64 NumPy mirrors vectorised over
  the samples, and ``figh_kinematic_regressor`` on the device;
* ``cartesian_to_SE3`` (``:545-561``), ``get_LMvariables`` (``:746-775``), ``update_joint_placement`` (``:1334-1362``) and
  ``calc_updated_fkm`` (``:1148-1331``), with the batched forms ``calc_updated_fkm_batch`` and ``fkm_jacobian_2point``
  (``figh_calib_fkm_batch``: every parameter vector of a forward-difference Jacobian in one launch);
* ``calculate_base_kinematics_regressor`` (``:1469-1561``): column elimination, independent column selection and base
  regressor of the kinematic regressor -- the second caller of ``eliminate_non_dynaffect`` / ``get_baseIndex`` /
  ``get_baseParams`` / ``build_baseRegressor``.  Parameter-name helpers ``get_geo_offset`` (``:301-331``) and
  ``get_joint_offset`` (``:252-298``) are mirrored because the base-parameter names are built from them.

Out of scope: data loading, several markers, the elastic ``non_geom`` terms of
``update_forward_kinematics[_2]`` and the Levenberg-Marquardt driver itself; posture selection is ``optimal_design``.
"""
import math

import numpy as np

from .. import _lib
from ..device import GpuMatrix
from ..model import JT_CONTINUOUS, JT_FREEFLYER, JT_PRISMATIC, JT_REVOLUTE, SE3
from ..tools.qrdecomposition import build_baseRegressor, get_baseIndex, get_baseParams
from ..tools.regressor import eliminate_non_dynaffect

TOL_QR = 1e-8

# name templates of the calibration parameters (calibration_tools.py:39-62)
FULL_PARAMTPL = ["d_px", "d_py", "d_pz", "d_phix", "d_phiy", "d_phiz"]
JOINT_OFFSETTPL = ["offsetPX", "offsetPY", "offsetPZ", "offsetRX", "offsetRY", "offsetRZ"]
ELAS_TPL = ["k_PX", "k_PY", "k_PZ", "k_RX", "k_RY", "k_RZ"]
EE_TPL = ["pEEx", "pEEy", "pEEz", "phiEEx", "phiEEy", "phiEEz"]
BASE_TPL = ["base_px", "base_py", "base_pz", "base_phix", "base_phiy", "base_phiz"]

_KINEMATIC_KEYS = ("NbSample", "start_frame", "end_frame", "measurability")


def get_joint_offset(model, joint_names):
    """{"offsetRZ_<joint>": 0, ...} -- one entry per joint degree of freedom, named after the joint model with
    "JointModel" replaced by "offset"; the second and later dofs of a joint carry their 1-based number
    (calibration_tools.py:252-298, including its special case for the model called "canopies").  Like the reference,
    the names come from ``model.names``, not from the argument."""
    names, joints = list(model.names[1:]), list(model.joints[1:])
    assert len(names) == len(joints), "Number of jointnames does not match number of joints! Please check\
        imported model."
    keys = []
    for name, joint in zip(names, joints):
        kind = joint.shortname()
        if model.name == "canopies" and "RevoluteUnaligned" in kind:
            kind = kind.replace("RevoluteUnaligned", "RZ")
        stem = kind.replace("JointModel", "offset")
        keys.extend((stem if dof == 0 else "%s%d" % (stem, dof + 1)) + "_" + name for dof in range(joint.nv))
    return dict.fromkeys(keys, 0)


def get_geo_offset(joint_names):
    """{"d_px_<joint>": 0, "d_py_<joint>": 0, ... "d_phiz_<joint>": 0} per joint (calibration_tools.py:301-331)."""
    return dict.fromkeys(("%s_%s" % (p, j) for j in joint_names for p in
                          ("d_px", "d_py", "d_pz", "d_phix", "d_phiy", "d_phiz")), 0)


# ---------------------------------------------------------------------------------------------------------------------
# SE(3) on batches: a placement is (R, p) with R (..., 3, 3) and p (..., 3); it maps child to parent coordinates
def rpy_to_matrix(rpy):
    """``pin.rpy.rpyToMatrix``: Rz(yaw) Ry(pitch) Rx(roll) for (..., 3) angles (roll, pitch, yaw)."""
    rpy = np.asarray(rpy, dtype=np.float64)
    r, p, y = rpy[..., 0], rpy[..., 1], rpy[..., 2]
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    R = np.empty(rpy.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = -sp, cp * sr, cp * cr
    return R


def matrix_to_rpy(R):
    """``pin.rpy.matrixToRpy``: the (roll, pitch, yaw) with pitch in [-pi/2, pi/2] of (..., 3, 3) rotations:
    pitch = atan2(-R20, sqrt(R00^2 + R10^2)), yaw = atan2(R10, R00), roll = atan2(R21, R22).  Within 1e-3 of gimbal lock
    (|pitch| = pi/2) the reference follows Eigen's ``eulerAngles``; that neighbourhood is outside this function's
    contract."""
    R = np.asarray(R, dtype=np.float64)
    out = np.empty(R.shape[:-2] + (3,))
    out[..., 1] = np.arctan2(-R[..., 2, 0], np.sqrt(R[..., 0, 0] * R[..., 0, 0] + R[..., 1, 0] * R[..., 1, 0]))
    out[..., 2] = np.arctan2(R[..., 1, 0], R[..., 0, 0])
    out[..., 0] = np.arctan2(R[..., 2, 1], R[..., 2, 2])
    return out


def _mul(A, B):
    """A . B for placements."""
    return A[0] @ B[0], (A[0] @ B[1][..., None])[..., 0] + A[1]


def _actinv(A, B):
    """A^-1 . B."""
    Rt = np.swapaxes(A[0], -1, -2)
    return Rt @ B[0], (Rt @ (B[1] - A[1])[..., None])[..., 0]


def _skew(p):
    S = np.zeros(p.shape[:-1] + (3, 3))
    S[..., 0, 1], S[..., 0, 2] = -p[..., 2], p[..., 1]
    S[..., 1, 0], S[..., 1, 2] = p[..., 2], -p[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -p[..., 1], p[..., 0]
    return S


def _action(M):
    """Ad(M) = [[R, skew(p) R], [0, R]] on (linear, angular) motions; the lower-left block is +0.0."""
    R, p = M
    X = np.zeros(R.shape[:-2] + (6, 6))
    X[..., :3, :3] = R
    X[..., :3, 3:] = _skew(p) @ R
    X[..., 3:, 3:] = R
    return X


def _se3_tuple(M):
    return np.array(M.rotation, dtype=np.float64), np.array(M.translation, dtype=np.float64)


def _joint_motion(joint, q):
    """M_j(q_j) for the (N, nq) configurations q."""
    N = q.shape[0]
    R = np.broadcast_to(np.eye(3), (N, 3, 3)).copy()
    p = np.zeros((N, 3))
    a = np.asarray(joint.axis, dtype=np.float64)
    if joint.jtype in (JT_REVOLUTE, JT_CONTINUOUS):
        if joint.jtype == JT_REVOLUTE:
            c, s = np.cos(q[:, joint.idx_q]), np.sin(q[:, joint.idx_q])
        else:
            c, s = q[:, joint.idx_q], q[:, joint.idx_q + 1]
        t = 1.0 - c  # Rodrigues for a unit axis, the statement the kernels use
        R[:, 0, 0] = 1.0 - t * (a[2] * a[2] + a[1] * a[1])
        R[:, 0, 1] = t * a[0] * a[1] - s * a[2]
        R[:, 0, 2] = t * a[0] * a[2] + s * a[1]
        R[:, 1, 0] = t * a[0] * a[1] + s * a[2]
        R[:, 1, 1] = 1.0 - t * (a[2] * a[2] + a[0] * a[0])
        R[:, 1, 2] = t * a[1] * a[2] - s * a[0]
        R[:, 2, 0] = t * a[0] * a[2] - s * a[1]
        R[:, 2, 1] = t * a[1] * a[2] + s * a[0]
        R[:, 2, 2] = 1.0 - t * (a[1] * a[1] + a[0] * a[0])
    elif joint.jtype == JT_PRISMATIC:
        p = q[:, joint.idx_q, None] * a[None, :]
    elif joint.jtype == JT_FREEFLYER:
        iq = joint.idx_q
        p = q[:, iq:iq + 3].copy()
        x, y, z, w = q[:, iq + 3], q[:, iq + 4], q[:, iq + 5], q[:, iq + 6]
        R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)
        R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)
        R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)
    return R, p


def _motion_subspace(joint):
    """S_j, 6 x nv_j: (0, axis) revolute / continuous, (axis, 0) prismatic, I6 free-flyer."""
    if joint.jtype == JT_FREEFLYER:
        return np.eye(6)
    S = np.zeros((6, 1))
    S[0 if joint.jtype == JT_PRISMATIC else 3:][:3, 0] = joint.axis
    return S


def _branch(model, j):
    """Joint ids from the root's child down to j (j = 0 or -1: empty)."""
    out = []
    while j > 0:
        out.append(int(j))
        j = model.parents[j]
    return out[::-1]


def _world_placements(model, q, joints):
    """{j: (A_j, oM_j)} for the joints listed and their ancestors: A_j = oM_parent(j) . jointPlacement_j,
    oM_j = A_j . M_j(q_j)."""
    need = set()
    for j in joints:
        need.update(_branch(model, j))
    N = q.shape[0]
    ident = (np.broadcast_to(np.eye(3), (N, 3, 3)), np.zeros((N, 3)))
    out = {0: (ident, ident)}
    for j in sorted(need):  # parents carry smaller ids
        A = _mul(out[model.parents[j]][1], _se3_tuple(model.jointPlacements[j]))
        out[j] = (A, _mul(A, _joint_motion(model.joints[j], q)))
    return out


def _as_configurations(model, q):
    q = np.asarray(q, dtype=np.float64)
    if q.ndim == 1:
        q = q[None, :]
    if q.ndim != 2 or q.shape[1] != model.nq:
        raise ValueError("expected (N, %d) configurations, got shape %r" % (model.nq, q.shape))
    return q


def _frame(model, frame_id):
    if not 0 <= int(frame_id) < len(model.frames):
        raise IndexError("frame %r is not in the model" % (frame_id,))
    f = model.frames[int(frame_id)]
    return f.parent, f.placement


def _named_frame(model, name):
    assert name in [f.name for f in model.frames], "{} does not exist.".format(name)
    return _frame(model, model.getFrameId(name))


def kinematic_regressor_batch(model, q, end_joint, end_placement, start_joint=-1, start_placement=None, support=None,
                              want_R=True, want_J=True):
    """(R, J) of shapes (N, 6, 6 (njoints - 1)) and (N, 6, nv) for the (N, nq) configurations q -- the float64 mirror of
    ``figh_kinematic_regressor`` and the one statement of the conventions.

    The end frame f sits on joint ``end_joint`` with placement ``end_placement``: oMf = oM_j . P_f.
    R[:, :, 6 (p - 1):6 p] = Ad(oMf^-1 . A_p) for every joint p of ``support`` (None: every joint from the root to the end
    joint) -- ``computeFrameKinematicRegressor(..., LOCAL)``: the frame's local twist per right-multiplied twist of joint
    p's placement.  J's columns of joint j on the root -> end path are Ad(oMf^-1 . oM_j) . S_j --
    ``computeFrameJacobian(..., LOCAL)``; with a start frame (``start_joint >= 0``) the same Jacobian of the start frame,
    in ITS local frame, is subtracted (``get_rel_jac``).  Everything else is +0.0."""
    q = _as_configurations(model, q)
    N = q.shape[0]
    end_branch = _branch(model, end_joint)
    start_branch = _branch(model, start_joint)
    support = list(end_branch) if support is None else [int(p) for p in support]
    world = _world_placements(model, q, [end_joint, start_joint] + support)
    oMf = _mul(world[max(int(end_joint), 0)][1], _se3_tuple(end_placement))
    R = J = None
    if want_R:
        R = np.zeros((N, 6, 6 * (model.njoints - 1)))
        for p in support:
            R[:, :, 6 * (p - 1):6 * p] = _action(_actinv(oMf, world[p][0]))
    if want_J:
        J = np.zeros((N, 6, model.nv))
        for j in end_branch:
            jm = model.joints[j]
            J[:, :, jm.idx_v:jm.idx_v + jm.nv] = _action(_actinv(oMf, world[j][1])) @ _motion_subspace(jm)
        if start_joint is not None and int(start_joint) >= 0:
            oMs = _mul(world[int(start_joint)][1], _se3_tuple(start_placement if start_placement is not None else SE3()))
            for j in start_branch:
                jm = model.joints[j]
                J[:, :, jm.idx_v:jm.idx_v + jm.nv] -= _action(_actinv(oMs, world[j][1])) @ _motion_subspace(jm)
    return R, J


def calculate_kinematics_model(q_i, model, data, param):
    """(model, data, R, J) for frame ``param["IDX_TOOL"]`` at one configuration (calibration_tools.py:1368-1392): R is
    ``computeFrameKinematicRegressor(..., LOCAL)`` (6 x 6 (njoints - 1)), J ``computeFrameJacobian(..., LOCAL)`` (6 x nv)."""
    joint, placement = _frame(model, param["IDX_TOOL"])
    R, J = kinematic_regressor_batch(model, q_i, joint, placement)
    return model, data, R[0], J[0]


def get_sup_joints(model, start_frame, end_frame):
    """Joint ids between two frames, ordered from the start to the end frame (calibration_tools.py:621-674, its three
    branch cases and its assertion kept)."""
    start_par = model.frames[model.getFrameId(start_frame)].parent
    end_par = model.frames[model.getFrameId(end_frame)].parent
    branch_s = model.supports[start_par].tolist()
    branch_e = model.supports[end_par].tolist()
    # remove 'universe' joint from branches
    if model.names[branch_s[0]] == "universe":
        branch_s.remove(branch_s[0])
    if model.names[branch_e[0]] == "universe":
        branch_e.remove(branch_e[0])
    shared_joints = list(set(branch_s) & set(branch_e))
    list_1 = [x for x in branch_s if x not in branch_e]
    list_1.reverse()
    list_2 = [y for y in branch_e if y not in branch_s]
    if shared_joints == []:  # case 2: the branches are separate
        sup_joints = list_1 + list_2
    elif shared_joints == branch_s:  # case 1: branch_s is part of branch_e
        sup_joints = [branch_s[-1]] + list_2
    else:
        assert shared_joints != branch_e, "End frame should be before start frame."
        sup_joints = list_1 + [shared_joints[-1]] + list_2  # case 3: the branches overlap
    return sup_joints


def get_rel_transform(model, data, start_frame, end_frame):
    """oM_start^-1 . oM_end from ``data.oMf`` (calibration_tools.py:592-618); ``frames_forward_kinematics`` fills it."""
    frames = [f.name for f in model.frames]
    assert start_frame in frames, "{} does not exist.".format(start_frame)
    assert end_frame in frames, "{} does not exist.".format(end_frame)
    oMsf = data.oMf[model.getFrameId(start_frame)]
    oMef = data.oMf[model.getFrameId(end_frame)]
    return SE3(oMsf.rotation.T @ oMef.rotation, oMsf.rotation.T @ (oMef.translation - oMsf.translation))


def frames_forward_kinematics(model, data, q):
    """``pin.framesForwardKinematics`` + ``pin.updateFramePlacements`` for one configuration: fills data.oMi / data.oMf."""
    q = _as_configurations(model, q)
    world = _world_placements(model, q, range(1, model.njoints))
    data.oMi = [SE3(world[j][1][0][0], world[j][1][1][0]) for j in range(model.njoints)]
    data.oMf = [data.oMi[f.parent] * f.placement for f in model.frames]
    return data


def get_rel_kinreg(model, data, start_frame, end_frame, q):
    """Kinematic regressor between two frames (calibration_tools.py:677-704): the blocks of the supporting joints only, each
    Ad(oMf^-1 . A_p) with the ABSOLUTE placement oMf of the end frame."""
    sup_joints = get_sup_joints(model, start_frame, end_frame)
    joint, placement = _frame(model, model.getFrameId(end_frame))
    R, _ = kinematic_regressor_batch(model, q, joint, placement, support=sup_joints, want_J=False)
    return R[0] if np.ndim(q) == 1 else R


def get_rel_jac(model, data, start_frame, end_frame, q):
    """J_end - J_start, each ``computeFrameJacobian(..., LOCAL)`` in its own frame (calibration_tools.py:707-740)."""
    sj, sp = _frame(model, model.getFrameId(start_frame))
    ej, ep = _frame(model, model.getFrameId(end_frame))
    _, J = kinematic_regressor_batch(model, q, ej, ep, sj, sp, want_R=False)
    return J[0] if np.ndim(q) == 1 else J


def random_configuration(model, rng):
    """One configuration drawn uniformly between the position limits (the role of ``pin.randomConfiguration``; not its
    bits): a continuous joint draws an angle in (-pi, pi] and stores (cos, sin), a free-flyer a uniform unit quaternion.  A
    joint with an infinite limit raises, as Pinocchio's does."""
    q = np.zeros(model.nq)
    lo, up = model.lowerPositionLimit, model.upperPositionLimit
    for jm, name in zip(model.joints[1:], model.names[1:]):
        iq = jm.idx_q
        if jm.jtype == JT_CONTINUOUS:
            ang = math.pi - rng.uniform(0.0, 2.0 * math.pi)
            q[iq], q[iq + 1] = math.cos(ang), math.sin(ang)
            continue
        n_lin = 3 if jm.jtype == JT_FREEFLYER else 1
        for k in range(iq, iq + n_lin):
            if not (np.isfinite(lo[k]) and np.isfinite(up[k])):
                raise RuntimeError("random_configuration: joint %s has an infinite position limit" % name)
            q[k] = rng.uniform(lo[k], up[k])
        if jm.jtype == JT_FREEFLYER:
            v = rng.standard_normal(4)
            q[iq + 3:iq + 7] = v / np.linalg.norm(v)
    return q


def random_configurations(model, rng, n):
    """``n`` configurations as ``random_configuration`` draws them, one array operation per joint (not the same stream of
    numbers as n single draws)."""
    q = np.zeros((n, model.nq))
    lo, up = model.lowerPositionLimit, model.upperPositionLimit
    for jm, name in zip(model.joints[1:], model.names[1:]):
        iq = jm.idx_q
        if jm.jtype == JT_CONTINUOUS:
            ang = math.pi - rng.uniform(0.0, 2.0 * math.pi, n)
            q[:, iq], q[:, iq + 1] = np.cos(ang), np.sin(ang)
            continue
        n_lin = 3 if jm.jtype == JT_FREEFLYER else 1
        for k in range(iq, iq + n_lin):
            if not (np.isfinite(lo[k]) and np.isfinite(up[k])):
                raise RuntimeError("random_configuration: joint %s has an infinite position limit" % name)
            q[:, k] = rng.uniform(lo[k], up[k], n)
        if jm.jtype == JT_FREEFLYER:
            v = rng.standard_normal((n, 4))
            q[:, iq + 3:iq + 7] = v / np.linalg.norm(v, axis=1)[:, None]
    return q


def _sample_rows(model, q, N):
    """The first N configurations of q for either route, checked before anything is launched: a host array (N, nq) or
    longer, or a ``GpuMatrix`` of at least N rows and exactly nq columns.  ValueError otherwise -- the kernels would read
    past the end of a shorter q."""
    if isinstance(q, GpuMatrix):
        rows, cols = q.rows, q.cols
    else:
        q = _as_configurations(model, np.asarray(q, dtype=np.float64))
        rows, cols = q.shape
    if cols != model.nq or rows < N:
        raise ValueError("q holds %d configurations of %d entries; param[\"NbSample\"] = %d needs at least that many rows of "
                         "nq = %d" % (rows, cols, N, model.nq))
    return q if isinstance(q, GpuMatrix) else q[:N]


def _meas_mask(measurability):
    comps = [c for c, state in enumerate(measurability) if state]
    if len(list(measurability)) != 6:
        raise ValueError("measurability has six entries (x, y, z, roll, pitch, yaw)")
    return comps, sum(1 << c for c in comps)


def _on_device(q, param):
    return isinstance(q, GpuMatrix) or bool(param.get("device_resident")) if hasattr(param, "get") else isinstance(q, GpuMatrix)


def _device_kinematic_regressor(model, q_dev, N, ej, ep, sj, sp, support, mask, want_R, want_J):
    """figh_kinematic_regressor into fresh device matrices; returns (R, J, rowsq_R, rowsq_J), host row sums of squares."""
    nmeas = bin(mask).count("1")
    handle = _device_handle(model)
    R = GpuMatrix.empty(nmeas * N, 6 * (model.njoints - 1)) if want_R else None
    J = GpuMatrix.empty(nmeas * N, model.nv) if want_J else None
    sq_R = _lib.DeviceArray((nmeas * N,)) if want_R else None
    sq_J = _lib.DeviceArray((nmeas * N,)) if want_J else None
    _lib.kinematic_regressor(handle, N, q_dev.ptr, q_dev.ld, ej, _placement12(ep), sj, _placement12(sp), support, mask,
                             R.ptr if want_R else None, R.ld if want_R else 0, J.ptr if want_J else None,
                             J.ld if want_J else 0, sq_R.ptr if want_R else None, sq_J.ptr if want_J else None)
    return R, J, (sq_R.to_host() if want_R else None), (sq_J.to_host() if want_J else None)


def _device_handle(model):
    """A fresh figh_model_t of this tree as it is NOW (``update_joint_placement`` edits placements in place, so a handle is
    never kept between calls); it is destroyed when the caller drops it."""
    return _lib.ModelHandle(model.to_flat())


def _placement12(M):
    out = np.zeros(12)
    if M is None:
        out[0] = out[4] = out[8] = 1.0
        return out
    out[:9] = np.asarray(M.rotation, dtype=np.float64).reshape(9)
    out[9:] = M.translation
    return out


def _drop_small_rows(W, rowsq):
    """np.delete(W, rows with 2-norm < 1e-6) on the device: nothing happens unless a row falls below the threshold."""
    keep = np.flatnonzero(~(np.sqrt(rowsq) < 1e-6))
    if len(keep) == W.rows:
        return W
    out = GpuMatrix.empty(len(keep), W.cols)
    _lib.gather_rows(W.ptr, W.ld, W.cols, _lib.DeviceArray.from_host(keep.astype(np.int32)), len(keep), out.ptr, out.ld)
    return out


def calculate_identifiable_kinematics_model(q, model, data, param):
    """The stacked Jacobian (``calib_model == "joint_offset"``) or kinematic regressor (``"full_params"``) over
    ``param["NbSample"]`` configurations (calibration_tools.py:1395-1466): row NbSample c + i holds row c of sample i when
    ``measurability[c]`` is true and zeros otherwise, and rows whose 2-norm is below 1e-6 are deleted in order.

    When ``np.any(q)`` is false the configurations are random: ``random_configurations`` seeded by ``param.get("seed", 0)``,
    its ``config_idx`` entries put into a COPY of ``param["q0"]`` (the reference aliases ``q0`` and overwrites it; the draws
    cannot be bit-equal to Pinocchio's generator, only the structural results built on them are comparable).  The
    reference allocates J with njoints - 1 columns, so it fails when nv differs; this function raises ValueError there.

    With a device the matrices are built by ``figh_kinematic_regressor`` (only the one asked for); a ``GpuMatrix`` q or
    ``param["device_resident"]`` returns a ``GpuMatrix``.  Without a device the float64 mirror runs."""
    N = int(param["NbSample"])
    q_is_dev = isinstance(q, GpuMatrix)
    if model.nv != model.njoints - 1:
        raise ValueError("could not broadcast input array from shape (%d,) into shape (%d,)" % (model.nv, model.njoints - 1))
    if not q_is_dev and not np.any(q):
        rng = np.random.default_rng(param.get("seed", 0))
        cfg = np.asarray(param["config_idx"], dtype=np.int64)
        qs = np.tile(np.asarray(param["q0"], dtype=np.float64).reshape(-1), (N, 1))
        qs[:, cfg] = random_configurations(model, rng, N)[:, cfg]
    else:
        qs = _sample_rows(model, q, N)
    comps, mask = _meas_mask(param["measurability"])
    if param["start_frame"] == "universe":
        ej, ep = _frame(model, param["IDX_TOOL"])
        sj, sp, support = -1, None, _branch(model, ej)
    else:
        support = get_sup_joints(model, param["start_frame"], param["end_frame"])
        sj, sp = _named_frame(model, param["start_frame"])
        ej, ep = _named_frame(model, param["end_frame"])
    want_J = param["calib_model"] == "joint_offset"
    want_R = param["calib_model"] == "full_params"
    if not (want_J or want_R):
        return None  # (the reference falls off its if / elif)
    if q_is_dev or _lib.device_count() > 0:
        q_dev = qs if q_is_dev else GpuMatrix.from_host(qs)
        R, J, sq_R, sq_J = _device_kinematic_regressor(model, q_dev, N, ej, ep, sj, sp, support, mask, want_R, want_J)
        W = _drop_small_rows(R, sq_R) if want_R else _drop_small_rows(J, sq_J)
        return W if _on_device(q, param) else W.numpy()
    R, J = kinematic_regressor_batch(model, qs, ej, ep, sj, sp, support, want_R=want_R, want_J=want_J)
    W = R if want_R else J
    full = np.zeros((6 * N, W.shape[2]))
    for c in comps:
        full[N * c:N * (c + 1)] = W[:, c, :]
    return full[~(np.sqrt(np.sum(full * full, axis=1)) < 1e-6)]


# ---------------------------------------------------------------------------------------------------------------------
# Levenberg-Marquardt tools
def cartesian_to_SE3(X):
    """[x, y, z, roll, pitch, yaw] -> SE3 (calibration_tools.py:545-561)."""
    X = np.array(X, dtype=np.float64).flatten("C")
    return SE3(rpy_to_matrix(X[3:6]), X[0:3])


def get_LMvariables(param, mode=0, seed=0):
    """(var, nvar): zeros (mode 0) or uniform in [-seed, seed] (mode 1) (calibration_tools.py:746-775)."""
    nvar = len(param["param_name"])
    if mode == 0:
        var = np.zeros(nvar)
    elif mode == 1:
        var = np.random.uniform(-seed, seed, nvar)
    return var, nvar


def update_joint_placement(model, joint_idx, xyz_rpy):
    """t' = t + xyz_rpy[0:3], R' = rpyToMatrix(matrixToRpy(R) + xyz_rpy[3:6]) on ``model.jointPlacements[joint_idx]``, in
    place (calibration_tools.py:1334-1362).  See ``matrix_to_rpy`` for the neighbourhood of gimbal lock."""
    xyz_rpy = np.asarray(xyz_rpy, dtype=np.float64)
    M = model.jointPlacements[joint_idx]
    updt_orientation = matrix_to_rpy(M.rotation) + xyz_rpy[3:6]
    M.translation = M.translation + xyz_rpy[0:3]
    M.rotation = rpy_to_matrix(updt_orientation)
    return model


def _lm_transforms(model, var, param, verbose=0):
    """The literal classification of calc_updated_fkm (calibration_tools.py:1175-1284): (wMo, eeMf, {joint: xyz_rpy})."""
    if param["calib_model"] == "full_params":
        axis_tpl = FULL_PARAMTPL
    elif param["calib_model"] == "joint_offset":
        axis_tpl = JOINT_OFFSETTPL
    assert len(var) == len(param["param_name"]), "Length of variables != length of params"
    param_dict = dict(zip(param["param_name"], var))
    updated_params = []
    base_param_incl = ee_param_incl = False
    for key in param_dict.keys():
        if "base" in key:
            base_param_incl = True
            break
    for key in param_dict.keys():
        if "EE" in key:
            ee_param_incl = True
            break
    if param["NbMarkers"] > 1:
        raise NotImplementedError("several markers (NbMarkers > 1) are outside this package's calibration path")
    if base_param_incl:
        base_tf = np.zeros(6)
        for key in param_dict.keys():
            for base_id, base_ax in enumerate(BASE_TPL):
                if base_ax in key:
                    base_tf[base_id] = param_dict[key]
                    updated_params.append(key)
        wMo = cartesian_to_SE3(base_tf)
    else:
        wMo = SE3()
    if ee_param_incl and param["NbMarkers"] == 1:
        for marker_idx in range(1, param["NbMarkers"] + 1):
            pee = np.zeros(6)
            ee_name = "EE"
            for key in param_dict.keys():
                if ee_name in key and str(marker_idx) in key:
                    for axis_pee_id, axis_pee in enumerate(EE_TPL):
                        if axis_pee in key:
                            if verbose == 1:
                                print("Updating [{}_{}] joint placement at axis {} with [{}]".format(
                                    ee_name, str(marker_idx), axis_pee, key))
                            pee[axis_pee_id] += param_dict[key]
                            updated_params.append(key)
            eeMf = cartesian_to_SE3(pee)
    else:
        eeMf = SE3()
    offsets = {}
    for j_id in param["actJoint_idx"]:
        xyz_rpy = np.zeros(6)
        j_name = model.names[j_id]
        for key in param_dict.keys():
            if j_name in key:
                for axis_id, axis in enumerate(axis_tpl):
                    if axis in key:
                        if verbose == 1:
                            print("Updating [{}] joint placement at axis {} with [{}]".format(j_name, axis, key))
                        xyz_rpy[axis_id] += param_dict[key]
                        updated_params.append(key)
        offsets[int(j_id)] = xyz_rpy
    assert len(updated_params) == len(list(param_dict.keys())), "Not all parameters are updated {} and {}".format(
        updated_params, list(param_dict.keys()))
    return wMo, eeMf, offsets


def _fkm_tables(model, var_batch, param, verbose=0):
    """Launch-uniform inputs of figh_calib_fkm_batch, formed in float64 on the host so that device and mirror start from
    the same bits: chain joints, their updated placements (B, n_chain, 12), wMo (B, 12) and eeMf (B, 12)."""
    chain = [int(j) for j in param["actJoint_idx"]]
    B = len(var_batch)
    placements, wMo, eeMf = np.zeros((B, len(chain), 12)), np.zeros((B, 12)), np.zeros((B, 12))
    for b, var in enumerate(var_batch):
        w, e, offsets = _lm_transforms(model, var, param, verbose)
        wMo[b], eeMf[b] = _placement12(w), _placement12(e)
        scratch = _PlacementsOnly([model.jointPlacements[j].copy() for j in chain])
        for k, j in enumerate(chain):
            update_joint_placement(scratch, k, offsets[j])
            placements[b, k] = _placement12(scratch.jointPlacements[k])
    return chain, placements, wMo, eeMf


class _PlacementsOnly:
    def __init__(self, placements):
        self.jointPlacements = placements


def _split_branches(model, start_joint, end_joint):
    """The joints of the start and of the end branch above their last common joint (each from that joint outwards)."""
    bs, be = _branch(model, start_joint), _branch(model, end_joint)
    k = 0
    while k < len(bs) and k < len(be) and bs[k] == be[k]:
        k += 1
    return bs[k:], be[k:]


def fkm_pose_batch(model, q, chain, placements, wMo, eeMf, start, end, measurability):
    """(B, n_meas * N) float64 mirror of ``figh_calib_fkm_batch``: per parameter vector b and pose i,
    wMf = wMo[b] . (cMs^-1 . cMe) . eeMf[b] with cMs / cMe the start / end frame seen from the last joint c both branches
    share (the factors below c cancel in oM_start^-1 . oM_end), the chain joints' placements taken from ``placements[b]``;
    the measured components of (translation, matrixToRpy(rotation)) go to out[b, k N + i]."""
    q = _as_configurations(model, q)
    N = q.shape[0]
    comps, _ = _meas_mask(measurability)
    (sj, sp), (ej, ep) = start, end
    up_s, up_e = _split_branches(model, sj, ej)
    slot = {j: k for k, j in enumerate(chain)}
    motions = {j: _joint_motion(model.joints[j], q) for j in up_s + up_e}
    out = np.zeros((len(placements), len(comps) * N))

    def seen_from_c(branch, b, P):
        M = (np.broadcast_to(np.eye(3), (N, 3, 3)), np.zeros((N, 3)))
        for j in branch:
            pl = placements[b, slot[j]] if j in slot else _placement12(model.jointPlacements[j])
            M = _mul(_mul(M, (pl[:9].reshape(3, 3), pl[9:])), motions[j])
        return _mul(M, P)

    for b in range(len(placements)):
        cMs = seen_from_c(up_s, b, _se3_tuple(sp) if sp is not None else (np.eye(3), np.zeros(3)))
        cMe = seen_from_c(up_e, b, _se3_tuple(ep))
        w, e = (wMo[b, :9].reshape(3, 3), wMo[b, 9:]), (eeMf[b, :9].reshape(3, 3), eeMf[b, 9:])
        wMf = _mul(_mul(w, _actinv(cMs, cMe)), e)
        loc = np.concatenate([wMf[1], matrix_to_rpy(wMf[0])], axis=1)  # (N, 6)
        for k, c in enumerate(comps):
            out[b, k * N:(k + 1) * N] = loc[:, c]
    return out


def calc_updated_fkm_batch(model, data, var_batch, q, param, verbose=0):
    """``calc_updated_fkm`` for the (B, nvar) parameter vectors ``var_batch`` at once: (B, calibration_index . N).  One
    launch of ``figh_calib_fkm_batch`` with a device (a ``GpuMatrix`` q or ``param["device_resident"]`` returns a
    ``GpuMatrix``), the float64 mirror without one.  The model is not touched."""
    var_batch = np.atleast_2d(np.asarray(var_batch, dtype=np.float64))
    N = int(param["NbSample"])
    chain, placements, wMo, eeMf = _fkm_tables(model, var_batch, param, verbose)
    start, end = _named_frame(model, param["start_frame"]), _named_frame(model, param["end_frame"])
    comps, mask = _meas_mask(param["measurability"])
    q_is_dev = isinstance(q, GpuMatrix)
    qs = _sample_rows(model, q, N)
    if q_is_dev or _lib.device_count() > 0:
        q_dev = qs if q_is_dev else GpuMatrix.from_host(qs)
        out = GpuMatrix.empty(len(var_batch), len(comps) * N)
        handle = _device_handle(model)  # (the joints off the chain take their placements from the model as it is now)
        _lib.calib_fkm_batch(handle, len(var_batch), N, q_dev.ptr, q_dev.ld, chain,
                             _lib.DeviceArray.from_host(placements.reshape(-1)), _lib.DeviceArray.from_host(wMo.reshape(-1)),
                             _lib.DeviceArray.from_host(eeMf.reshape(-1)), end[0], _placement12(end[1]), start[0],
                             _placement12(start[1]), mask, out.ptr, out.ld)
        return out if _on_device(q, param) else out.numpy()
    return fkm_pose_batch(model, qs, chain, placements, wMo, eeMf, start, end, param["measurability"])


def calc_updated_fkm(model, data, var, q, param, verbose=0):
    """The Levenberg-Marquardt model function (calibration_tools.py:1148-1331): the measured pose components of the marker
    for every configuration, PEE[k, i] flattened C-order to index k N + i, with the joint placements, the base transform
    (``base_*`` parameters) and the marker transform (``*EE*`` parameters) updated by ``var``.  The classification of
    ``param["param_name"]`` by substrings and its two assertions are the reference's.  This function works on copies of the
    placements, so the caller's model is never changed: the reference's update / revert pair and its two ``!=`` assertions
    have no counterpart.  ``NbMarkers > 1`` raises NotImplementedError; joint elasticity is not modelled."""
    out = calc_updated_fkm_batch(model, data, np.asarray(var, dtype=np.float64)[None, :], q, param, verbose)
    if isinstance(out, GpuMatrix):
        return out
    return out[0]


def fkm_jacobian_2point(model, data, var, q, param, rel_step=None):
    """(m, nvar) forward-difference Jacobian of ``calc_updated_fkm`` at ``var`` from ONE batch of nvar + 1 parameter
    vectors, with SciPy's '2-point' rule: h = rel_step sign(x) max(1, |x|), sign(0) = 1, rel_step = sqrt(eps) by default,
    and the step re-read as (x + h) - x.  Fits ``scipy.optimize.least_squares(jac=...)``."""
    x0 = np.asarray(var, dtype=np.float64).reshape(-1)
    rel = np.finfo(np.float64).eps ** 0.5 if rel_step is None else rel_step
    h = rel * ((x0 >= 0).astype(float) * 2 - 1) * np.maximum(1.0, np.abs(x0))
    batch = np.tile(x0, (len(x0) + 1, 1))
    for i in range(len(x0)):
        batch[i + 1, i] += h[i]
    F = np.asarray(calc_updated_fkm_batch(model, data, batch, q, param))
    dx = batch[np.arange(1, len(x0) + 1), np.arange(len(x0))] - x0
    return ((F[1:] - F[0]) / dx[:, None]).T


def calculate_base_kinematics_regressor(q, model, data, param, tol_qr=TOL_QR, kinematics_model=None):
    """(Rrand_b, R_b, R_e, paramsrand_base, paramsrand_e) -- calibration_tools.py:1469-1561; the base parameter names are
    appended to ``param["param_name"]`` and the three shapes are printed, as the reference does.
    ``kinematics_model(q, model, data, param)`` builds the kinematic regressors: None means this module's
    ``calculate_identifiable_kinematics_model`` when ``param`` carries the kinematic keys ("NbSample", "start_frame",
    "end_frame", "measurability"), and NotImplementedError otherwise; a callable is used as given.  The four regressor
    reductions run on the device."""
    if kinematics_model is None and all(k in param for k in _KINEMATIC_KEYS):
        kinematics_model = calculate_identifiable_kinematics_model
    if kinematics_model is None:
        raise NotImplementedError("pass kinematics_model=calculate_identifiable_kinematics_model: the kinematic "
                                  "regressor is part of the calibration subsystem (needs Pinocchio), not of this path")
    names = list(model.names[1:])
    candidates = {"joint_offset": get_joint_offset(model, names), "full_params": get_geo_offset(names)}
    # regressor over random configurations (fixed base: the model draws them itself, hence []), and over the given
    # ones when there are any
    R_random = kinematics_model(q if param["free_flyer"] else [], model, data, param)
    R_given = kinematics_model(q, model, data, param) if np.any(np.array(q)) else R_random
    if param["calib_model"] not in candidates:  # the reference leaves geo_params_sel unbound
        raise UnboundLocalError("local variable 'geo_params_sel' referenced before assignment")
    selected = candidates[param["calib_model"]]
    # random data decide which parameters are identifiable and which of them are independent ...
    Rrand_e, paramsrand_e = eliminate_non_dynaffect(R_random, selected, tol_e=1e-6)
    idx_base = get_baseIndex(Rrand_e, paramsrand_e, tol_qr=tol_qr)
    Rrand_b, paramsrand_base, _ = get_baseParams(Rrand_e, paramsrand_e, tol_qr=tol_qr)
    # ... the given data are reduced the same way (their own base set is computed and dropped, as in the reference)
    # and restricted to the columns chosen on the random data
    R_e, params_e = eliminate_non_dynaffect(R_given, selected, tol_e=1e-6)
    get_baseParams(R_e, params_e, tol_qr=tol_qr)
    R_b = build_baseRegressor(R_e, idx_base)
    param["param_name"].extend(paramsrand_e[j] for j in idx_base)
    print("shape of full regressor, reduced regressor, base regressor: ", R_random.shape, Rrand_e.shape, Rrand_b.shape)
    return Rrand_b, R_b, R_e, paramsrand_base, paramsrand_e
