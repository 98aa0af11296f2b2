"""CPU suite of the free-flyer real-data functions (identification_tools.quaternion_log, rotation_vector_to_quaternion,
filter_free_flyer, transport_wrench): the NumPy mirrors -- the functions' definitions on the host -- against the exact
restatement of freeflyer_common in every regime, the conventions a wrong implementation would get wrong, the row pairing of
the orientation filter against a literal transcription of the script, and the refusals.  The device runs the same checks in
test_freeflyer_entrywise.py."""
import numpy as np
import pytest

import freeflyer_common as fc
from figaroh_plus_amd.identification import identification_tools as it


# ------------------------------------------------------------------------------------------- mirrors against the restatement
@pytest.mark.parametrize("regime", fc.LOG_REGIMES)
def test_log_mirror_against_the_restatement(regime, record_property):
    quat = fc.log_inputs(regime)
    got = it.quaternion_log_mirror(quat)
    r, zeros_ok = fc.ratio(got, fc.log_reference(regime))
    record_property("ratio", r)
    print("log %-12s ratio %.4f" % (regime, r))
    assert zeros_ok and r <= fc.C_TOL_LOG
    if regime == "n_0":  # three zeros, all of them +0.0
        assert np.all(got == 0.0) and not np.any(np.signbit(got))
    # q and -q give the same vector, bit for bit -- except at w = 0, where sgn(0) = sgn(-0) = +1 turns -q into -r: theta = pi
    # there, and r and -r are the same rotation
    assert np.array_equal(it.quaternion_log_mirror(-quat), -got if regime == "w_0" else got)


@pytest.mark.parametrize("regime", fc.EXP_REGIMES)
def test_exp_mirror_against_the_restatement(regime, record_property):
    rotvec, ref = fc.exp_inputs(regime)
    ex = fc.exp_reference(regime)
    # the restatement itself says that no sample sits on a decision: d away from cos(pi / 4), Eigen's ties away
    excluded = (np.abs(ex.info["d"] - fc.KEEP_ABOVE) <= fc.MARGIN) | (ex.info["tie"] <= fc.MARGIN)
    assert np.count_nonzero(excluded) == 0
    mode = np.arange(len(rotvec)) % 4
    d = ex.info["d"]
    assert np.all(d[mode == 0] > 0.999) and np.all(d[mode == 1] < -0.8) and np.all(np.abs(d[mode == 2]) < 0.6)
    got = it.rotation_vector_to_quaternion_mirror(rotvec, ref)
    r, zeros_ok = fc.ratio(got, ex)
    record_property("ratio", r)
    print("exp %-20s ratio %.4f" % (regime, r))
    assert zeros_ok and r <= fc.C_TOL_EXP


def test_exp_regimes_reach_both_sign_cases_and_d_above_one():
    """Every reference mode meets both of Eigen's sign cases, a canonical quaternion with a negative scalar part occurs, and
    some references have d > 1 (their float64 norm exceeds 1): the restatement keeps there, so the checks above demand it."""
    vector = np.concatenate([fc.exp_reference(r).info["vector_case"] for r in fc.EXP_REGIMES])
    mode = np.concatenate([np.arange(fc.N_REF) % 4 for _ in fc.EXP_REGIMES])
    for k in range(4):
        assert np.any(vector[mode == k]) and np.any(~vector[mode == k])
    d = np.concatenate([fc.exp_reference(r).info["d"] for r in fc.EXP_REGIMES])
    assert np.count_nonzero(d > 1.0) >= 8
    rotvec, ref = fc.exp_inputs("beyond_pi")
    th = np.linalg.norm(rotvec, axis=1)
    assert np.any(np.abs(np.cos(th / 2)) > 0.5) and np.any(np.abs(np.cos(th / 2)) < 0.5) and np.all(np.cos(th / 2) < 0)
    keep = mode[:fc.N_REF] == 0  # d = 1 up to rounding: kept, so the output is Eigen's representative, dot product +1
    out = it.rotation_vector_to_quaternion_mirror(rotvec, ref)
    assert np.all(np.sum(out[keep] * ref[keep], axis=1) > 0.999)


@pytest.mark.parametrize("name", fc.TRANSPORT_CASES)
@pytest.mark.parametrize("inverse", [False, True])
def test_transport_mirror_against_the_restatement(name, inverse, record_property):
    model, joint = fc.transport_case(name)
    q, F = fc.transport_inputs(name)
    ex = fc.transport_reference(name, inverse)
    worst = 0.0
    for lin in ("sample", "stacked"):
        for lout in ("sample", "stacked"):
            got = it.transport_wrench_mirror(model, q, fc.to_layout(F, lin), joint, inverse, lin, lout)
            r, zeros_ok = fc.ratio(fc.from_layout(got, len(q), lout), ex)
            worst = max(worst, r)
            assert zeros_ok and r <= fc.C_TOL_TRN
    record_property("ratio", worst)
    print("transport %-22s inverse %d ratio %.4f" % (name, inverse, worst))


def test_transport_round_trip_and_names():
    """action then inverse action gives the wrench back to rounding; a joint goes by name or id; joint 0 is the identity."""
    model, joint = fc.transport_case("human_root")
    q, F = fc.transport_inputs("human_root")
    world = it.transport_wrench_mirror(model, q, F, "root_joint", False, "sample", "stacked")
    back = it.transport_wrench_mirror(model, q, world, joint, True, "stacked", "sample")
    assert np.abs(back - F).max() <= 1e-12 * np.abs(F).max()
    assert np.array_equal(it.transport_wrench_mirror(model, q, F, 0, False, "sample", "sample"), F)


def test_freeflyer_c_oracle_matches_the_recorded_figures():
    """C_ORACLE_* are what this CPU measures over exactly the rows of the GPU suite, and C_TOL_* follow from them by the
    project's rule (the power of two in [8, 16] x C_ORACLE).  The mirrors' libm may differ from the one that recorded the
    figures by an ulp here and there: the recomputed figures must give the same C_TOL."""
    c_log, c_exp, c_trn = fc.measure_c_oracle()
    print("C_ORACLE_LOG %.6g  C_ORACLE_EXP %.6g  C_ORACLE_TRN %.6g" % (c_log, c_exp, c_trn))
    for got, recorded, tol in ((c_log, fc.C_ORACLE_LOG, fc.C_TOL_LOG), (c_exp, fc.C_ORACLE_EXP, fc.C_TOL_EXP),
                               (c_trn, fc.C_ORACLE_TRN, fc.C_TOL_TRN)):
        assert abs(got - recorded) <= 0.05 * recorded
        assert tol == fc.tol_rule(recorded) == fc.tol_rule(got)
        assert 8.0 * recorded <= tol <= 16.0 * recorded


# ------------------------------------------------------------------------------------------------------ planted conventions
# A plant is judged row by row on the first rows of a regime: when every single row misses the bound, every prefix -- every
# shape of the GPU suite, N = 1 included -- does.
PLANT_ROWS = 8


def _every_row_fails(got, ex, tol):
    return all(fc.ratio(got[i:i + 1], ex.row(i))[0] > tol for i in range(len(got)))


@pytest.mark.parametrize("plant", fc.LOG_PLANTS)
def test_planted_log_conventions_fail(plant):
    """wxyz order everywhere (at n = 0 it reads w as a vector component); the dropped sgn(w) wherever w < 0 (with n = 0 or
    w = 0 there is no sign to drop)."""
    for regime in fc.LOG_REGIMES:
        quat = fc.log_inputs(regime)[:4 * PLANT_ROWS]
        if plant == "no_sign":
            if regime in ("n_0", "w_0"):
                continue
            quat = quat[quat[:, 3] < 0][:PLANT_ROWS]
            assert len(quat) >= 4
        else:
            quat = quat[:PLANT_ROWS]
        assert _every_row_fails(it.quaternion_log_mirror(quat), fc.exact_log(quat, plant), fc.C_TOL_LOG), regime


def test_planted_exp_convention_fails():
    for regime in fc.EXP_REGIMES:
        rotvec, ref = (x[:PLANT_ROWS] for x in fc.exp_inputs(regime))
        got = it.rotation_vector_to_quaternion_mirror(rotvec, ref)
        assert _every_row_fails(got, fc.exact_exp(rotvec, ref, "wxyz"), fc.C_TOL_EXP), regime


# where a planted convention computes something else.  wxyz: a free-flyer on the path.  moment_first: p != 0 (with p = 0
# force and moment are rotated alike).  cross_before_rotation: the action only, p != 0.  placement_right: a placement on the
# path that is not the identity.  iMo: everywhere.
DISTINGUISHES = {
    "wxyz": ("human_root", "tree_freeflyer", "placed_tree_freeflyer"),
    "moment_first": ("human_root", "tree_freeflyer", "placed_tree_freeflyer", "placed_tree_last"),
    "cross_before_rotation": ("human_root", "tree_freeflyer", "placed_tree_freeflyer", "placed_tree_last"),
    "iMo": fc.TRANSPORT_CASES,
    "placement_right": ("human_root", "placed_tree_freeflyer", "placed_tree_last"),
}


@pytest.mark.parametrize("plant", fc.TRANSPORT_PLANTS)
def test_planted_transport_conventions_fail(plant):
    assert "human_root" in DISTINGUISHES[plant]
    for name in DISTINGUISHES[plant]:
        model, joint = fc.transport_case(name)
        q, F = fc.transport_inputs(name)
        for inverse in (False, True):
            if plant == "cross_before_rotation" and inverse:
                continue
            got = it.transport_wrench_mirror(model, q[:PLANT_ROWS], F[:PLANT_ROWS], joint, inverse, "sample", "sample")
            planted = fc.exact_transport(name, inverse, plant, PLANT_ROWS)
            assert _every_row_fails(got, planted, fc.C_TOL_TRN), (name, inverse)


# --------------------------------------------------------------------------------------------- the orientation filter
def _script_param():
    return {"ts": 0.01, "cut_off_frequency_butterworth": 15.0}


def _script_transcription(q_mocap, params_settings, lo, nq):
    """examples/human/identification.py:330-374 statement by statement, with the mirrors in the place of pin.log3 and of
    pin.Quaternion(pin.exp3(.)) + the sign test, and SciPy's filtfilt in the place of low_pass_filter_data (which is what
    the reference's function calls).  ``lo``: the column of the quaternion's x (3 in the script)."""
    from scipy import signal

    def low_pass_filter_data(data, param, nbutter=5):
        b, a = signal.butter(nbutter, param["ts"] * param["cut_off_frequency_butterworth"] / 2, "low")
        padlen = 3 * (max(len(b), len(a)) - 1)
        data = signal.filtfilt(b, a, data, axis=0, padtype="odd", padlen=padlen)
        nbord = 5 * nbutter
        data = np.delete(data, np.s_[0:nbord], axis=0)
        data = np.delete(data, np.s_[data.shape[0] - nbord:data.shape[0]], axis=0)
        return data

    rotvec_list = []
    for ii in range(len(q_mocap)):
        quat = np.array([q_mocap[ii, lo], q_mocap[ii, lo + 1], q_mocap[ii, lo + 2], q_mocap[ii, lo + 3]])
        rotvec_ii = it.quaternion_log_mirror(quat)[0]
        rotvec_list.append(rotvec_ii)
    rotvec_nofilt = np.array(rotvec_list)
    for ii in range(rotvec_nofilt.shape[1]):
        if ii == 0:
            rotvec = low_pass_filter_data(rotvec_nofilt[:, ii], params_settings, 5)
        else:
            rotvec = np.column_stack((rotvec, low_pass_filter_data(rotvec_nofilt[:, ii], params_settings, 5)))
    quat_filt = np.zeros((rotvec.shape[0], 4))
    for ii in range(rotvec.shape[0]):
        rotvec_ii = rotvec[ii, :]
        quat_ref = np.array([q_mocap[ii, lo], q_mocap[ii, lo + 1], q_mocap[ii, lo + 2], q_mocap[ii, lo + 3]])
        quat_filt[ii, :] = it.rotation_vector_to_quaternion_mirror(rotvec_ii, quat_ref)[0]
    for ii in range(nq):
        if ii == 0:
            q_m = low_pass_filter_data(q_mocap[:, ii], params_settings, 5)
        else:
            q_m = np.column_stack((q_m, low_pass_filter_data(q_mocap[:, ii], params_settings, 5)))
    q_m[:, lo:lo + 4] = quat_filt
    return q_m


@pytest.mark.parametrize("name,n", [("human_root", 171), ("tree_freeflyer", 90)])
def test_filter_row_pairing_and_trimming_against_the_script(name, n):
    """filter_free_flyer_mirror is the script: 25 rows trimmed per border, row ii of the filtered rotation vector paired with
    RAW row ii (not ii + 25), quaternion columns overwritten, every other column low-pass filtered."""
    model, _ = fc.transport_case(name)
    q = fc.mocap_like(model, n, 5)
    lo = [j.idx_q + 3 for j in model.joints[1:] if j.jtype == 3][0]
    got = it.filter_free_flyer_mirror(model, q, _script_param())
    want = _script_transcription(q, _script_param(), lo, model.nq)
    assert got.shape == want.shape == (n - 50, model.nq)
    assert np.array_equal(got, want)
    # the pairing matters on this trajectory: against row ii + 25 some rows come out with the other sign
    rotvec = it.quaternion_log_mirror(q[:, lo:lo + 4])
    from scipy import signal
    b, a = signal.butter(5, 0.01 * 15.0 / 2, "low")
    filt = signal.filtfilt(b, a, rotvec, axis=0, padtype="odd", padlen=15)[25:-25]
    shifted = it.rotation_vector_to_quaternion_mirror(filt, q[25:n - 25, lo:lo + 4])
    assert not np.array_equal(shifted, got[:, lo:lo + 4])
    assert np.allclose(np.abs(np.sum(shifted * got[:, lo:lo + 4], axis=1)), 1.0, atol=1e-12)  # (the same rotations)
    with pytest.raises(ValueError):
        it.filter_free_flyer_mirror(model, q[:, :-1], _script_param())


# ------------------------------------------------------------------------------------------------------------- refusals
def test_shape_and_argument_refusals_raise_before_any_launch(monkeypatch):
    """Every refusal of the public functions is a ValueError raised on the host: no entry of the library is reached."""
    def forbidden(*args, **kw):
        raise AssertionError("a refused call reached the library")

    for entry in ("quat_log", "rotvec_to_quat", "wrench_transport"):
        monkeypatch.setattr(it._lib, entry, forbidden)
    monkeypatch.setattr(it._lib.DeviceArray, "from_host", classmethod(forbidden))
    model, _ = fc.transport_case("human_root")
    q, F = (x[:9] for x in fc.transport_inputs("human_root"))
    for fn in (it.quaternion_log, it.quaternion_log_mirror):
        for bad in (np.zeros((5, 3)), np.zeros((0, 4)), np.zeros((2, 2, 4))):
            with pytest.raises(ValueError):
                fn(bad)
    for fn in (it.rotation_vector_to_quaternion, it.rotation_vector_to_quaternion_mirror):
        for rv, ref in ((np.zeros((5, 4)), np.zeros((5, 4))), (np.zeros((5, 3)), np.zeros((5, 3))),
                        (np.zeros((5, 3)), np.zeros((4, 4))), (np.zeros((0, 3)), np.zeros((0, 4)))):
            with pytest.raises(ValueError):
                fn(rv, ref)
    for fn in (it.transport_wrench, it.transport_wrench_mirror):
        for kw in (dict(q=q[:, :-1]), dict(q=q[:0], wrench=F[:0]), dict(wrench=F[:8]), dict(wrench=F.reshape(-1)),
                   dict(wrench=F, layout_in="stacked"), dict(layout_in="blocked"), dict(layout_out="joint-major"),
                   dict(joint="no_such_joint"), dict(joint=model.njoints), dict(joint=-1)):
            args = dict(dict(q=q, wrench=F, joint="root_joint", layout_in="sample", layout_out="stacked"), **kw)
            with pytest.raises(ValueError):
                fn(model, args["q"], args["wrench"], joint=args["joint"], layout_in=args["layout_in"],
                   layout_out=args["layout_out"])
    for fn in (it.filter_free_flyer, it.filter_free_flyer_mirror):
        with pytest.raises(ValueError):
            fn(model, q[:, :-1], _script_param())


def test_raw_entries_refuse_before_they_need_a_device():
    """figh_quat_log and figh_rotvec_to_quat look at their arguments before they look for a device: FIGH_ERR_INVALID with a
    reason, nothing launched, whether or not there is a GPU (the addresses are never dereferenced on a refusal)."""
    from figaroh_plus_amd import _lib

    import __graft_entry__ as entry
    import os
    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    a, b, c = 1 << 20, 2 << 20, 3 << 20  # stand-ins for device addresses, 1 MB apart
    cases = [(_lib.quat_log, (a, 0, 4, b, 3), "at least one sample"), (_lib.quat_log, (a, 5, 3, b, 3), "leading dimension"),
             (_lib.quat_log, (a, 5, 4, b, 2), "leading dimension"), (_lib.quat_log, (a, 5, 4, a + 8, 3), "overlaps"),
             (_lib.quat_log, (None, 5, 4, b, 3), "NULL"),
             (_lib.rotvec_to_quat, (a, 0, 3, b, 4, c, 4), "at least one sample"),
             (_lib.rotvec_to_quat, (a, 5, 2, b, 4, c, 4), "leading dimension"),
             (_lib.rotvec_to_quat, (a, 5, 3, b, 3, c, 4), "leading dimension"),
             (_lib.rotvec_to_quat, (a, 5, 3, b, 4, c, 3), "leading dimension"),
             (_lib.rotvec_to_quat, (a, 5, 3, b, 4, b + 8, 4), "overlaps"),    # overlaps the reference, is not the reference
             (_lib.rotvec_to_quat, (a, 5, 3, b, 8, b, 4), "overlaps"),        # the same pointer, another leading dimension
             (_lib.rotvec_to_quat, (a, 5, 3, b, 4, a, 4), "overlaps")]        # over the rotation vectors
    for fn, args, reason in cases:
        with pytest.raises(_lib.FighError) as e:
            fn(*args)
        assert e.value.code == _lib.ERR_INVALID and reason in str(e.value), (args, str(e.value))
