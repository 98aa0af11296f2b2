"""CPU suite of the geometric calibration path: the conventions of the kinematic regressor and Jacobian derived from first
principles at 50 digits, the float64 mirrors of calibration/calibration_tools.py against the exact restatement of
kinematics_common.py entry by entry, planted convention errors, and the host logic around them.  The device entries are
checked by test_kinematics_entrywise.py with the same restatement and the constants measured here."""
import copy
import json

import mpmath
import numpy as np
import pytest

import kinematics_common as kc
from figaroh_plus_amd.calibration import calibration_tools as ct
from figaroh_plus_amd.model import SE3, Model

mpf = mpmath.mpf
N_HOST = 6          # samples per case of the entrywise checks
H = mpf(10) ** -25  # step of the first-principles derivatives


# ------------------------------------------------------------------------------------------------ 1. first principles
def _mp(M):
    return mpmath.matrix([[x.v for x in row] for row in M])


def _exp6(xi):
    """exp of the twist (v, w) as a 4 x 4 mpmath matrix (series coefficients for the tiny angles used here)."""
    v, w = mpmath.matrix(xi[:3]), mpmath.matrix(xi[3:])
    th2 = sum(x * x for x in w)
    a, b, c = 1 - th2 / 6, mpf(1) / 2 - th2 / 24, mpf(1) / 6 - th2 / 120
    K = mpmath.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = mpmath.eye(3) + a * K + b * K * K
    p = (mpmath.eye(3) + b * K + c * K * K) * v
    M = mpmath.eye(4)
    M[0:3, 0:3] = R
    M[0:3, 3] = p
    return M


def _log6(M):
    """log of a placement within 1e-24 of the identity, to second order: (p - w x p / 2, w), w = vee(R - R^T) / 2."""
    w = [(M[2, 1] - M[1, 2]) / 2, (M[0, 2] - M[2, 0]) / 2, (M[1, 0] - M[0, 1]) / 2]
    p = [M[0, 3], M[1, 3], M[2, 3]]
    wxp = [w[1] * p[2] - w[2] * p[1], w[2] * p[0] - w[0] * p[2], w[0] * p[1] - w[1] * p[0]]
    return [p[k] - wxp[k] / 2 for k in range(3)] + w


def _inv(M):
    R = M[0:3, 0:3].T
    out = mpmath.eye(4)
    out[0:3, 0:3] = R
    out[0:3, 3] = -R * M[0:3, 3]
    return out


def _frame_placement(model, q, joint, placement, placement_post=None, motion_post=None):
    """oMf by plain composition of 4 x 4 matrices: prod (jointPlacement_j [. post] . M_j(q_j) [. post]) . P_f."""
    M = mpmath.eye(4)
    for j in kc.branch(model, joint):
        M = M * _mp(kc.hom_of_se3(model.jointPlacements[j]))
        if placement_post and j in placement_post:
            M = M * placement_post[j]
        M = M * _mp(kc.joint_hom(model.joints[j], q))
        if motion_post and j in motion_post:
            M = M * motion_post[j]
    return M * _mp(kc.hom_of_se3(placement if placement is not None else SE3()))


def _dof_step(joint, k):
    """Right factor of M_j(q_j) that integrates its k-th degree of freedom by H."""
    xi = [mpf(0)] * 6
    if joint.jtype == 3:
        xi[k] = H
    else:
        off = 0 if joint.jtype == 1 else 3
        for d in range(3):
            xi[off + d] = H * joint.axis[d]
    return _exp6(xi)


# The float64 models are rigid only to rounding: rotations orthogonal, axes and quaternions of unit length to 1e-16, and the
# statements under test invert a placement by transposing.  A derivative taken through true inverses differs from them by
# that 1e-16, relatively.  The first-principles check therefore runs on the IDEAL geometry next to each model: every rotation
# projected onto SO(3), every axis, (cos, sin) pair and quaternion normalised, at 50 digits.
def _project_so3(R):
    for _ in range(4):  # Newton's iteration for the polar factor: the distance to SO(3) squares each time
        R = (R + (R.T) ** -1) / 2
    return R


def _ideal_hom_of_se3(M):
    R = _project_so3(mpmath.matrix([[mpf(float(x)) for x in row] for row in M.rotation]))
    rows = [[kc.V(R[r, c]) if R[r, c] != 0 else kc.ZERO for c in range(3)] for r in range(3)]
    return kc.hom(rows, [kc.V(x) if x != 0.0 else kc.ZERO for x in M.translation])


class _IdealJoint:
    def __init__(self, jm):
        self.jtype, self.idx_q, self.idx_v, self.nv = jm.jtype, jm.idx_q, jm.idx_v, jm.nv
        a = [mpf(float(x)) for x in jm.axis]
        n = mpmath.sqrt(sum(x * x for x in a))
        self.axis = [x / n for x in a] if n != 0 else a


class _IdealModel:
    def __init__(self, m):
        self.joints = [_IdealJoint(jm) for jm in m.joints]
        self.parents, self.jointPlacements, self.njoints, self.nv = m.parents, m.jointPlacements, m.njoints, m.nv


def _ideal_configuration(m, q):
    out = [mpf(float(x)) for x in q]
    for jm in m.joints[1:]:
        span = range(jm.idx_q, jm.idx_q + 2) if jm.jtype == 2 else range(jm.idx_q + 3, jm.idx_q + 7) if jm.jtype == 3 else ()
        n = mpmath.sqrt(sum(out[k] ** 2 for k in span)) if span else 1
        for k in span:
            out[k] = out[k] / n
    return out


@pytest.mark.parametrize("name", kc.CASE_NAMES)
def test_conventions_from_first_principles(name, monkeypatch):
    """For every joint p between the root and the end frame: jointPlacement_p <- jointPlacement_p exp6(h d) moves the frame
    by log6(oMf^-1 oMf') / h = R[:, block p] d, and integrating each degree of freedom of joint j by h moves it by column
    of J (for a start frame: minus the same for the start frame) -- to 1e-20, h = 1e-25.  Pins LOCAL against WORLD, motion
    against force action, which placement is perturbed, the (linear, angular) order and the column offsets.  A supporting
    joint on the start frame's branch does not move the end frame; its block is the reference's statement
    (get_rel_kinreg): the twist d of a body at A_p seen from the end frame, exp6(h R d) = oMf^-1 A_p exp6(h d) A_p^-1 oMf."""
    monkeypatch.setattr(kc, "hom_of_se3", _ideal_hom_of_se3)
    case = kc.get_case(name)
    q = _ideal_configuration(case.model, case.configurations(1, seed=11)[0])
    m = _IdealModel(case.model)
    rng = np.random.default_rng(5)
    end_path = kc.branch(m, case.end_joint)
    full = copy.copy(case)
    full.model = m
    full.support = sorted(set(end_path) | set(case.support))
    R, J = kc.exact_regressor_sample(full, q)
    oMf = _frame_placement(m, q, case.end_joint, case.end_placement)
    for p in full.support:
        d = rng.standard_normal(6)
        d /= np.linalg.norm(d)
        dm = [mpf(float(x)) for x in d]
        if p in end_path:
            moved = _frame_placement(m, q, case.end_joint, case.end_placement, placement_post={p: _exp6([H * x for x in dm])})
            twist = _log6(_inv(oMf) * moved)
        else:
            A_p = _frame_placement(m, q, m.parents[p], None) * _mp(kc.hom_of_se3(m.jointPlacements[p]))
            twist = _log6(_inv(oMf) * A_p * _exp6([H * x for x in dm]) * _inv(A_p) * oMf)
        for r in range(6):
            want = sum(R[r][6 * (p - 1) + c].v * dm[c] for c in range(6))
            assert abs(twist[r] / H - want) <= mpf(10) ** -20, (name, p, r)
    oMs = _frame_placement(m, q, case.start_joint, case.start_placement) if case.start_joint >= 0 else None
    for j in sorted(set(end_path) | set(kc.branch(m, case.start_joint))):
        jm = m.joints[j]
        for k in range(jm.nv):
            step = {j: _dof_step(jm, k)}
            twist = _log6(_inv(oMf) * _frame_placement(m, q, case.end_joint, case.end_placement, motion_post=step))
            if oMs is not None:
                moved = _frame_placement(m, q, case.start_joint, case.start_placement, motion_post=step)
                twist = [a - b for a, b in zip(twist, _log6(_inv(oMs) * moved))]
            for r in range(6):
                assert abs(twist[r] / H - J[r][jm.idx_v + k].v) <= mpf(10) ** -20, (name, j, k, r)


# ---------------------------------------------------------------------------------- 2. mirror against exact, 3. plants
@pytest.fixture(scope="module")
def exact():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = kc.regressor_reference(name, N_HOST)
        return cache[name]

    return get


def _mirror_regressor(case, q):
    return ct.kinematic_regressor_batch(case.model, q, case.end_joint, case.end_placement, case.start_joint,
                                        case.start_placement, case.support)


def _regressor_ratio(case, exact_RJ, R, J):
    _, Re, Je = exact_RJ
    r1, z1 = kc.ratio(R, Re.hi, Re.scale)
    r2, z2 = kc.ratio(J, Je.hi, Je.scale)
    return max(r1, r2), z1 and z2


@pytest.mark.parametrize("name", kc.CASE_NAMES)
def test_regressor_mirror_against_exact(name, exact, record_property):
    case = kc.get_case(name)
    q = exact(name)[0]
    R, J = _mirror_regressor(case, q)
    worst, zeros_ok = _regressor_ratio(case, exact(name), R, J)
    record_property("ratio", worst)
    print("%s: mirror / exact ratio %.3f" % (name, worst))
    assert zeros_ok, "a structural zero is not +0.0"
    assert worst <= kc.C_KIN
    # the lower-left 3 x 3 of every block, the columns off the support and the Jacobian columns off the paths: exact zeros
    off = [p for p in range(1, case.model.njoints) if p not in case.support]
    for p in case.support:
        assert np.all(R[:, 3:, 6 * (p - 1):6 * (p - 1) + 3] == 0.0)
    for p in off:
        assert not np.any(R[:, :, 6 * (p - 1):6 * p]) and not np.any(np.signbit(R[:, :, 6 * (p - 1):6 * p]))


def _fkm_setup(case, n, seed):
    param = kc.fkm_param(case, n)
    var = kc.fkm_offsets(len(param["param_name"]), 1, seed)[0]
    return param, var


def _tables(case, var, param):
    chain, placements, wMo, eeMf = ct._fkm_tables(case.model, var[None, :], param)
    return chain, placements[0], wMo[0], eeMf[0]


def _pick_seed(case, q, seeds=range(20, 40)):
    """The first seed whose offsets keep every pose and every updated placement away from gimbal lock -- asserted by the
    tests on the exact values; the seed is chosen, no case is dropped."""
    for seed in seeds:
        param, var = _fkm_setup(case, len(q), seed)
        hi, sc, worst = kc.exact_pee(case, q, *_tables(case, var, param), param["measurability"])
        worst = max(worst, kc.exact_tables(case, var)[3])
        if worst <= kc.PITCH_LIMIT:
            return seed, param, var, hi, sc, worst
    raise AssertionError("no seed in %r keeps %s away from gimbal lock" % (seeds, case.name))


def _pee_configurations(case, n):
    """Configurations whose end-frame pitch stays below the limit: the first n of a longer draw that satisfy it at zero
    offsets (the exact check on the offsets actually used is made by the caller)."""
    q = case.configurations(8 * n, seed=17)
    param = kc.fkm_param(case, 1)
    zero = np.zeros(len(param["param_name"]))
    keep = []
    for qi in q:
        _, _, worst = kc.exact_pee(case, qi[None, :], *_tables(case, zero, param), param["measurability"])
        if worst <= kc.PITCH_LIMIT - 0.15:
            keep.append(qi)
        if len(keep) == n:
            break
    assert len(keep) == n
    return np.array(keep)


@pytest.fixture(scope="module")
def pee_exact():
    cache = {}

    def get(name):
        if name not in cache:
            case = kc.get_case(name)
            q = _pee_configurations(case, N_HOST)
            cache[name] = (q,) + _pick_seed(case, q)
        return cache[name]

    return get


@pytest.mark.parametrize("name", kc.CASE_NAMES)
def test_fkm_mirror_against_exact(name, pee_exact, record_property, monkeypatch):
    monkeypatch.setattr(ct._lib, "device_count", lambda: 0)  # the float64 mirror, whatever the machine has
    case = kc.get_case(name)
    q, seed, param, var, hi, sc, worst_pitch = pee_exact(name)
    assert worst_pitch <= kc.PITCH_LIMIT
    before = [M.copy() for M in case.model.jointPlacements]
    got = ct.calc_updated_fkm(case.model, None, var, q, param)
    assert got.shape == (6 * len(q),)
    worst, _ = kc.ratio(got, hi, sc)
    tables = _table_ratio(case, var, param)
    record_property("ratio", max(worst, tables))
    print("%s: PEE mirror / exact ratio %.3f, tables %.3f (seed %d)" % (name, worst, tables, seed))
    assert worst <= kc.C_PEE and tables <= kc.C_TAB
    for a, b in zip(before, case.model.jointPlacements):  # the caller's model is never mutated
        assert np.array_equal(a.rotation, b.rotation) and np.array_equal(a.translation, b.translation)


def _table_ratio(case, var, param):
    """Largest ratio of the mirror's launch-uniform tables against their exact restatement."""
    worst, zeros_ok = kc.table_ratio(case, var, param)
    assert zeros_ok
    return worst


def test_c_oracle_matches_the_recorded_figures(exact, pee_exact, monkeypatch):
    """C_KIN / C_PEE / C_TAB are the powers of two in [8, 16] x the recorded C_ORACLE figures (kinematics_common.py,
    DESIGN.md; measured by kinematics_common.measure_c_oracle over the shapes of the GPU suite), and the largest mirror / exact
    ratio over the few samples of this module is of their size and no larger."""
    monkeypatch.setattr(ct._lib, "device_count", lambda: 0)
    kin = pee = tab = 0.0
    for name in kc.CASE_NAMES:
        case = kc.get_case(name)
        kin = max(kin, _regressor_ratio(case, exact(name), *_mirror_regressor(case, exact(name)[0]))[0])
        q, seed, param, var, hi, sc, _ = pee_exact(name)
        pee = max(pee, kc.ratio(ct.calc_updated_fkm(case.model, None, var, q, param), hi, sc)[0])
        tab = max(tab, _table_ratio(case, var, param))
    print("C_ORACLE_KIN measured %.6g, C_ORACLE_PEE measured %.6g, C_ORACLE_TAB measured %.6g" % (kin, pee, tab))
    for C, oracle, recorded in ((kc.C_KIN, kin, kc.C_ORACLE_KIN), (kc.C_PEE, pee, kc.C_ORACLE_PEE),
                                (kc.C_TAB, tab, kc.C_ORACLE_TAB)):
        assert 8 * recorded <= C <= 16 * recorded and np.log2(C) == int(np.log2(C))
        assert 0.25 * recorded <= oracle <= 1.001 * recorded  # (fewer samples than the recorded figure's: no larger)


def _force_action(M):
    R, p = M
    X = np.zeros(R.shape[:-2] + (6, 6))
    X[..., :3, :3] = R
    X[..., 3:, :3] = ct._skew(p) @ R
    X[..., 3:, 3:] = R
    return X


def _joint_in_place_of_placement(orig):
    def planted(model, q, joints):
        return {j: (oM, oM) for j, (A, oM) in orig(model, q, joints).items()}
    return planted


def _rpy_xyz(rpy):
    rpy = np.asarray(rpy, dtype=np.float64)
    r, p, y = rpy[..., 0], rpy[..., 1], rpy[..., 2]
    one, zero = np.ones_like(r), np.zeros_like(r)

    def mat(rows):
        return np.stack([np.stack(row, axis=-1) for row in rows], axis=-2)

    Rx = mat([[one, zero, zero], [zero, np.cos(r), -np.sin(r)], [zero, np.sin(r), np.cos(r)]])
    Ry = mat([[np.cos(p), zero, np.sin(p)], [zero, one, zero], [-np.sin(p), zero, np.cos(p)]])
    Rz = mat([[np.cos(y), -np.sin(y), zero], [np.sin(y), np.cos(y), zero], [zero, zero, one]])
    return Rx @ Ry @ Rz


REGRESSOR_PLANTS = ("world_frame", "force_action", "joint_for_placement", "block_shift", "angular_linear")
FKM_PLANTS = ("rpy_xyz", "ee_left")


@pytest.mark.parametrize("plant", REGRESSOR_PLANTS)
@pytest.mark.parametrize("name", kc.CASE_NAMES)
def test_planted_regressor_errors_are_caught(name, plant, exact, monkeypatch):
    """Each wrong convention, planted into the mirror, fails the entrywise check at every shape."""
    case = kc.get_case(name)
    q = exact(name)[0]
    if plant == "world_frame":
        monkeypatch.setattr(ct, "_actinv", lambda A, B: B)
    elif plant == "force_action":
        monkeypatch.setattr(ct, "_action", _force_action)
    elif plant == "joint_for_placement":
        monkeypatch.setattr(ct, "_world_placements", _joint_in_place_of_placement(ct._world_placements))
    R, J = _mirror_regressor(case, q)
    if plant == "block_shift":
        R = np.roll(R, 6, axis=2)
    elif plant == "angular_linear":
        R, J = R[:, [3, 4, 5, 0, 1, 2], :], J[:, [3, 4, 5, 0, 1, 2], :]
    _, Re, Je = exact(name)
    worst, zeros_ok = kc.ratio_fast(R, Re.hi, Re.scale)
    if plant == "joint_for_placement":  # (R only: the Jacobian never reads A_p)
        assert worst > kc.C_KIN or not zeros_ok
        return
    worst_J, zeros_J = kc.ratio_fast(J, Je.hi, Je.scale)
    assert worst > kc.C_KIN or not zeros_ok
    if plant != "block_shift":  # (a shift of R's blocks leaves J alone)
        assert worst_J > kc.C_KIN or not zeros_J


@pytest.mark.parametrize("plant", FKM_PLANTS)
@pytest.mark.parametrize("name", kc.CASE_NAMES)
def test_planted_fkm_errors_are_caught(name, plant, pee_exact, monkeypatch):
    """Rx Ry Rz in rpyToMatrix fails the check of the tables; the marker transform on the left fails the check of the pose."""
    case = kc.get_case(name)
    q, seed, param, var, hi, sc, _ = pee_exact(name)
    if plant == "rpy_xyz":
        monkeypatch.setattr(ct, "rpy_to_matrix", _rpy_xyz)
        assert _table_ratio(case, var, param) > kc.C_TAB
        return
    chain, placements, wMo, eeMf = ct._fkm_tables(case.model, var[None, :], param)
    e, w = (eeMf[0, :9].reshape(3, 3), eeMf[0, 9:]), (wMo[0, :9].reshape(3, 3), wMo[0, 9:])
    Rl, pl = ct._mul(e, w)  # wMf = eeMf . wMo . oMee
    wMo = np.concatenate([Rl.reshape(-1), pl])[None, :]
    eeMf = ct._placement12(None)[None, :]
    got = ct.fkm_pose_batch(case.model, q, chain, placements, wMo, eeMf, ct._named_frame(case.model, case.start_frame),
                            ct._named_frame(case.model, case.end_frame), param["measurability"])[0]
    assert kc.ratio_fast(got, hi, sc)[0] > kc.C_PEE


# ------------------------------------------------------------------------------------------------------ 4. host logic
@pytest.mark.parametrize("route", ["mirror", "device"])
def test_short_or_misshaped_q_raises_before_any_launch(route, monkeypatch):
    """param["NbSample"] larger than q, or q of another width, is a ValueError on both routes, for host arrays and for a
    GpuMatrix alike: the check runs before the route is chosen, so nothing is launched on a q the kernels would read past."""
    from figaroh_plus_amd.device import GpuMatrix

    monkeypatch.setattr(ct._lib, "device_count", lambda: 0 if route == "mirror" else 1)
    case = kc.get_case("ur10_tool")
    m = case.model
    q = case.configurations(4)
    fparam = kc.fkm_param(case, 5)
    var = np.zeros(len(fparam["param_name"]))
    resident_short = GpuMatrix(None, 4, m.nq)        # (never dereferenced: the check comes first)
    resident_narrow = GpuMatrix(None, 5, m.nq - 1)
    for bad in (q, q[0], q[:, :5], np.zeros((5, m.nq + 1)) + 0.1, resident_short, resident_narrow):
        for calib_model in ("full_params", "joint_offset"):
            with pytest.raises(ValueError):
                ct.calculate_identifiable_kinematics_model(bad, m, None, _ident_param(case, 5, (1,) * 6, calib_model))
        with pytest.raises(ValueError):
            ct.calc_updated_fkm(m, None, var, bad, fparam)
        with pytest.raises(ValueError):
            ct.calc_updated_fkm_batch(m, None, var[None, :], bad, fparam)
    monkeypatch.setattr(ct._lib, "device_count", lambda: 0)  # a longer q is cut to NbSample rows, as the reference reads it
    long_q = case.configurations(7)
    assert np.array_equal(ct.calc_updated_fkm(m, None, var, long_q, dict(fparam, NbSample=4)),
                          ct.calc_updated_fkm(m, None, var, long_q[:4], dict(fparam, NbSample=4)))



def test_frames_of_the_host_model(tmp_path):
    m = kc.get_case("tiago_tool").model
    assert m.frames[0].name == "universe" and m.frames[0].parent == 0
    assert [f.name for f in m.frames[:m.njoints]] == m.names and [f.parent for f in m.frames[:m.njoints]] == list(range(m.njoints))
    assert m.getFrameId("tool") == m.njoints and m.getFrameId("no such frame") == len(m.frames)
    assert m.supports[m.getJointId("arm_2_joint")].tolist() == [0, 13, 14, 15]
    assert "frames" not in m.to_flat()  # to_flat keeps exactly its keys; the shipped models are not regenerated
    m.save_flat(str(tmp_path / "tiago.json"))
    with open(tmp_path / "tiago.json") as f:
        flat = json.load(f)
    P = m.frames[-1].placement
    flat["frames"] = [{"name": "tool", "parent": m.frames[-1].parent,
                       "placement": [float(x) for x in P.rotation.reshape(-1)] + [float(x) for x in P.translation]}]
    again = Model.from_flat(flat)
    assert again.getFrameId("tool") == m.njoints and np.array_equal(again.frames[-1].placement.rotation, P.rotation)


def test_get_sup_joints_three_cases_and_assertion():
    m = kc.get_case("tiago_tool").model
    arm = list(range(14, 21))
    assert ct.get_sup_joints(m, "torso_lift_joint", "tool") == [13] + arm             # case 1
    assert ct.get_sup_joints(m, "head_2_joint", "tool") == [24, 23, 13] + arm          # case 3
    assert ct.get_sup_joints(m, "wheel_left_joint", "tool") == [10, 9, 13] + arm       # case 2: no joint shared
    with pytest.raises(AssertionError, match="End frame should be before start frame."):
        ct.get_sup_joints(m, "tool", "torso_lift_joint")
    t = kc.get_case("talos_wrists").model
    assert ct.get_sup_joints(t, "left_tool", "right_tool") == list(range(22, 14, -1)) + list(range(24, 31))


def _ident_param(case, n, mask, calib_model):
    m = case.model
    return {"NbSample": n, "calibration_index": int(sum(mask)), "start_frame": case.start_frame, "end_frame": case.end_frame,
            "IDX_TOOL": m.getFrameId(case.end_frame), "measurability": [bool(x) for x in mask], "calib_model": calib_model,
            "q0": np.zeros(m.nq), "config_idx": [m.joints[j].idx_q for j in case.support], "free_flyer": False,
            "param_name": []}


@pytest.mark.parametrize("name", ["ur10_tool", "tiago_torso_arm7", "tiago_head_arm7"])
@pytest.mark.parametrize("mask", kc.MASKS)
def test_row_stacking_measurability_and_zero_rows(name, mask, monkeypatch):
    """calculate_identifiable_kinematics_model against a literal per-sample loop (calibration_tools.py:1432-1466)."""
    monkeypatch.setattr(ct._lib, "device_count", lambda: 0)
    case = kc.get_case(name)
    m, n = case.model, 5
    q = case.configurations(n, seed=23)
    for calib_model in ("full_params", "joint_offset"):
        param = _ident_param(case, n, mask, calib_model)
        R = np.zeros((6 * n, 6 * (m.njoints - 1)))
        J = np.zeros((6 * n, m.njoints - 1))
        for i in range(n):
            if case.start_frame == "universe":
                _, _, Ri, Ji = ct.calculate_kinematics_model(q[i], m, None, param)
            else:
                Ri = ct.get_rel_kinreg(m, None, case.start_frame, case.end_frame, q[i])
                Ji = ct.get_rel_jac(m, None, case.start_frame, case.end_frame, q[i])
            for j, state in enumerate(param["measurability"]):
                if state:
                    R[n * j + i, :] = Ri[j, :]
                    J[n * j + i, :] = Ji[j, :]
        R = np.delete(R, [r for r in range(R.shape[0]) if np.linalg.norm(R[r]) < 1e-6], axis=0)
        J = np.delete(J, [r for r in range(J.shape[0]) if np.linalg.norm(J[r]) < 1e-6], axis=0)
        got = ct.calculate_identifiable_kinematics_model(q, m, None, param)
        assert np.array_equal(got, R if calib_model == "full_params" else J)


def test_random_configurations_and_q0_is_copied(monkeypatch):
    monkeypatch.setattr(ct._lib, "device_count", lambda: 0)
    case = kc.get_case("ur10_tool")
    param = _ident_param(case, 7, (1, 1, 1, 1, 1, 1), "full_params")
    q0 = param["q0"].copy()
    a = ct.calculate_identifiable_kinematics_model([], case.model, None, param)
    b = ct.calculate_identifiable_kinematics_model(np.zeros((7, 6)), case.model, None, dict(param, seed=0))
    c = ct.calculate_identifiable_kinematics_model([], case.model, None, dict(param, seed=1))
    assert a.shape == (42, 36) and np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(param["q0"], q0)  # the reference overwrites q0; this mirror does not
    rng = np.random.default_rng(0)
    m = case.model
    for _ in range(20):
        q = ct.random_configuration(m, rng)
        assert np.all(q >= m.lowerPositionLimit) and np.all(q <= m.upperPositionLimit)
    tiago = kc.get_case("tiago_tool").model
    wheel = tiago.joints[tiago.getJointId("wheel_left_joint")]
    q = ct.random_configuration(tiago, rng)
    assert abs(np.hypot(q[wheel.idx_q], q[wheel.idx_q + 1]) - 1.0) < 1e-15
    with pytest.raises(RuntimeError, match="infinite position limit"):
        ct.random_configuration(kc.get_case("human_wrist").model, rng)
    with pytest.raises(ValueError):  # nv != njoints - 1: the reference's J assignment fails
        tree = kc.get_case("tree_tool")
        ct.calculate_identifiable_kinematics_model(tree.configurations(3), tree.model, None,
                                                   _ident_param(tree, 3, (1,) * 6, "joint_offset"))


def test_fkm_classification_and_assertions(monkeypatch):
    monkeypatch.setattr(ct._lib, "device_count", lambda: 0)
    case = kc.get_case("ur10_tool")
    q = case.configurations(3, seed=2)
    param = kc.fkm_param(case, 3)
    var = kc.fkm_offsets(len(param["param_name"]), 1, 4)[0]
    wMo, eeMf, offsets = ct._lm_transforms(case.model, var, param)
    assert np.array_equal(wMo.translation, var[0:3]) and np.array_equal(eeMf.translation, var[-6:-3])
    assert np.array_equal(wMo.rotation, ct.rpy_to_matrix(var[3:6]))
    for k, j in enumerate(kc.active_joints(case)):
        assert np.array_equal(offsets[j], var[6 + 6 * k:12 + 6 * k])
    with pytest.raises(AssertionError, match="Length of variables != length of params"):
        ct.calc_updated_fkm(case.model, None, var[:-1], q, param)
    stray = dict(param, param_name=param["param_name"] + ["d_px_no_such_joint"])
    with pytest.raises(AssertionError, match="Not all parameters are updated"):
        ct.calc_updated_fkm(case.model, None, np.append(var, 0.0), q, stray)
    with pytest.raises(NotImplementedError):
        ct.calc_updated_fkm(case.model, None, var, q, dict(param, NbMarkers=2))
    # joint_offset names: one rotation offset about z per joint lands in slot 5 of the joint's (x y z roll pitch yaw)
    po = kc.fkm_param(case, 3, calib_model="joint_offset")
    vo = kc.fkm_offsets(len(po["param_name"]), 1, 4)[0]
    _, _, off = ct._lm_transforms(case.model, vo, po)
    assert all(np.array_equal(off[j], [0, 0, 0, 0, 0, vo[6 + k]]) for k, j in enumerate(kc.active_joints(case)))
    assert ct.get_LMvariables(param)[1] == len(var) and not np.any(ct.get_LMvariables(param)[0])
    # masks pick the rows of the full pose in order
    full = ct.calc_updated_fkm(case.model, None, var, q, param).reshape(6, 3)
    part = ct.calc_updated_fkm(case.model, None, var, q, dict(param, measurability=[True, False, False, True, False, True],
                                                              calibration_index=3))
    assert np.array_equal(part, full[[0, 3, 5]].reshape(-1))


@pytest.mark.parametrize("name", ["ur10_tool", "tiago_head_arm7"])
def test_fkm_at_zero_is_plain_forward_kinematics(name, monkeypatch):
    monkeypatch.setattr(ct._lib, "device_count", lambda: 0)
    case = kc.get_case(name)
    m = case.model
    q = _pee_configurations(case, 4)
    param = kc.fkm_param(case, 4)
    got = ct.calc_updated_fkm(m, None, np.zeros(len(param["param_name"])), q, param).reshape(6, 4)
    data = m.createData()
    for i in range(4):
        ct.frames_forward_kinematics(m, data, q[i])
        M = ct.get_rel_transform(m, data, case.start_frame, case.end_frame)
        want = np.concatenate([M.translation, ct.matrix_to_rpy(M.rotation)])
        # matrixToRpy(rpyToMatrix(.)) of the unchanged placements is the identity only to rounding
        assert np.allclose(got[:, i], want, rtol=0, atol=1e-13)


def test_fkm_jacobian_2point_is_scipys(monkeypatch):
    monkeypatch.setattr(ct._lib, "device_count", lambda: 0)
    from scipy.optimize._numdiff import approx_derivative

    case = kc.get_case("tiago_torso_arm7")
    q = _pee_configurations(case, 3)
    param = kc.fkm_param(case, 3, mask=(1, 1, 1, 0, 0, 1))
    var = kc.fkm_offsets(len(param["param_name"]), 1, 6)[0]
    var[3] = 0.0   # sign(0) = 1
    var[7] = -1.5  # |x| > 1 scales the step
    J = ct.fkm_jacobian_2point(case.model, None, var, q, param)
    ref = approx_derivative(lambda x: ct.calc_updated_fkm(case.model, None, x, q, param), var, method="2-point")
    assert J.shape == (12, len(var)) and np.array_equal(J, ref)


def _restated_base(W, names, tol_qr=1e-8):
    """eliminate_non_dynaffect + get_baseIndex restated with NumPy: columns whose squared norm reaches 1e-6, then the
    columns whose diagonal entry of R in np.linalg.qr exceeds tol_qr."""
    keep = [c for c in range(W.shape[1]) if np.sum(W[:, c] ** 2) >= 1e-6]
    Rq = np.linalg.qr(W[:, keep], mode="r")
    base = [k for k in range(len(keep)) if abs(Rq[k, k]) > tol_qr]
    return keep, [names[c] for c in keep], base


@pytest.mark.parametrize("name,calib_model", [("ur10_tool", "full_params"), ("tiago_torso_arm7", "joint_offset")])
def test_identifiable_model_structure(name, calib_model, monkeypatch):
    """The mirror's regressor over N = 200 random configurations: every column of a joint off the support is eliminated
    and the base count is that of the restatement -- the structural facts calculate_base_kinematics_regressor builds on
    (its own run, which needs the device's reductions, is compared with the same restatement in
    test_kinematics_entrywise.py)."""
    monkeypatch.setattr(ct._lib, "device_count", lambda: 0)
    case = kc.get_case(name)
    m = case.model
    param = _ident_param(case, 200, (1,) * 6, calib_model)
    assert m.nv == m.njoints - 1  # (TIAGo's continuous wheels have one degree of freedom each)
    W = ct.calculate_identifiable_kinematics_model([], m, None, param)
    names = list((ct.get_geo_offset(m.names[1:]) if calib_model == "full_params" else ct.get_joint_offset(m, m.names[1:])))
    assert W.shape[1] == len(names)
    keep, kept_names, base = _restated_base(W, names)
    for p in range(1, m.njoints):
        cols = range(6 * (p - 1), 6 * p) if calib_model == "full_params" else [m.joints[p].idx_v]
        if p not in case.support:
            assert not any(c in keep for c in cols), m.names[p]
    if calib_model == "full_params":
        assert len(keep) == 36 and len(base) < 36  # a serial chain's 6 n placement errors are not independent
    else:
        assert [names[c] for c in keep] == kept_names and len(base) == len(keep) == len(case.support)


def test_kinematics_model_none_rule(monkeypatch):
    """kinematics_model=None: the package's own function when param carries the kinematic keys, today's
    NotImplementedError otherwise; a callable is used as given."""
    case = kc.get_case("ur10_tool")
    m = case.model
    bare = {"free_flyer": False, "calib_model": "full_params", "param_name": []}
    with pytest.raises(NotImplementedError, match="pass kinematics_model=calculate_identifiable_kinematics_model"):
        ct.calculate_base_kinematics_regressor(np.zeros((2, 6)), m, None, bare)
    calls = []

    def own(q, model, data, param):
        calls.append(len(q))
        raise KeyError("reached the package's own function")

    monkeypatch.setattr(ct, "calculate_identifiable_kinematics_model", own)
    with pytest.raises(KeyError, match="own function"):
        ct.calculate_base_kinematics_regressor(np.zeros((2, 6)), m, None, dict(_ident_param(case, 2, (1,) * 6, "full_params")))
    assert calls == [0]

    def given(q, model, data, param):
        raise IndexError("reached the callable")

    with pytest.raises(IndexError, match="the callable"):
        ct.calculate_base_kinematics_regressor(np.zeros((2, 6)), m, None, bare, kinematics_model=given)
