"""GPU suite: the batched, W-free excitation objective for serial chains (figh_regressor_tsqr_batch_fused, figh_fused.hip).

One launch builds the regressor tiles of B trajectories in LDS and factors the base columns there; one launch per merge
level turns every trajectory's triangles (+ R_stack) into its R.  Checked here: every returned triangle column by column
against the long-double Gram of the W that the two-launch path (build_regressor_basic, pinned on the reference's goldens)
writes for that trajectory's samples; objective_cond_batch against objective_cond and against np.linalg.cond of the
oracle's host W_b; the launch counts (one level-0 launch, no K1 launch, merge launches independent of B); every refusal of
the entry, and the fall-back of excitation.py behind it.
"""
import numpy as np
import pytest

import qr_graded_common as qg
from qr_graded_common import TOL_BACKWARD

pytestmark = pytest.mark.gpu

# the smallest trajectory the entry takes (figh_fused.hip: kFusedBatchMinSamples, one full sample tile)
N_FLOOR = 64
FLAG_SETS = [dict(has_friction=f, has_actuator_inertia=i, has_joint_offset=o)
             for f in (False, True) for i in (False, True) for o in (False, True)]


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    qg.check_longdouble()
    return _lib


def _slices(B, n_per, cus):
    """Slices per trajectory the entry launches (figh_fused.hip, fused_batch_slices): one round of the chip, at most one
    slice per sample tile, 1 when B alone fills the chip."""
    return max(1, min(-(-n_per // 64), cus // B))


def _merge_levels(S, ncons, r, stacked):
    """Merge launches of the entry: 512 stacked rows per workgroup and level (launch_fused_batch)."""
    rows, levels = S * ncons * r + (r if stacked else 0), 0
    while True:
        levels += 1
        nb = -(-rows // 512)
        if nb == 1:
            return levels
        rows = nb * r


def _consumers(nj, r):
    """Consumer waves per workgroup (launch_fused_batch: what fits next to two tile buffers in 160 KB, at most six)."""
    nc = 14 * nj
    psize = 64 * (nc + 2) + 64 * nj + 2 * 64 * nj + ((nc + 7) // 8) * 8 + 4
    pad = 64 - r
    skip = sum(16 * max(3 - (kp >> 4), 0) for kp in range(pad))
    tri = 80 + 256 * 6 - skip
    return min(6, (160 * 1024 // 8 - 2 * psize) // tri)


def _robot(name):
    if name == "ur10":
        from conftest import Golden
        return Golden("cfg2_ur10").robot()
    from test_gpu_parity import _synthetic_chain
    return _synthetic_chain(int(name[5:]))


def _param(**flags):
    p = dict(is_joint_torques=True, is_external_wrench=False, has_friction=False, has_actuator_inertia=False,
             has_joint_offset=False, force_torque=None)
    p.update(flags)
    return p


def _trajectories(robot, B, n_per, seed):
    """B different trajectories (amplitudes grow with b: a mix-up of trajectories changes every column norm)."""
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        q, v, a = sample_inputs(robot.model, n_per, rng, 1.5, 2, 5)
        s = 1.0 + 0.5 * b / max(B - 1, 1)
        out.append((q, s * v, s * a))
    return out


def _base_columns_numpy(robot, param, seed=5):
    """Columns of W with a non-zero norm whose R diagonal is non-negligible (get_index_eliminate + get_baseParams on a
    host QR of the two-launch path's W), at most the 64 the entry factors (63 with seven joints: LDS, figh.h)."""
    from figaroh_plus_amd.tools.regressor import build_regressor_basic
    q, v, a = _trajectories(robot, 1, 400, seed)[0]
    W = build_regressor_basic(robot, q, v, a, dict(param))
    keep = np.flatnonzero(np.sqrt((W * W).sum(axis=0)) > 1e-6)
    d = np.abs(np.diag(np.linalg.qr(W[:, keep], mode="r")))
    return keep[d > 1e-6 * d.max()][:63 if robot.model.nv == 7 else 64].astype(np.int32)


def _gram_ld(A):
    Al = np.asarray(A, dtype=np.longdouble)
    return Al.T @ Al


def _check_gram(R, G, record_property, tag):
    """Backward metric of a kernel-built W's triangle against a long-double Gram (test_qr_structured_graded._check_gram)."""
    assert np.array_equal(R, np.triu(R))
    b = qg.backward_err(R, G)
    record_property(tag + ":backward", "%.3e" % b)
    print("%s: backward %.3e" % (tag, b))
    assert b <= TOL_BACKWARD, "%s: backward %.3e > %.1e" % (tag, b, TOL_BACKWARD)


def _run_entry(lib, robot, param, trajs, cols, R_stack=None):
    """The new entry through _lib directly: B x r x r, exactly as the device wrote it."""
    from figaroh_plus_amd.tools.regressor import regressor_flags
    mode, flags, _ = regressor_flags(param)
    assert mode == lib.MODE_JOINT_TORQUE
    B, n_per, r = len(trajs), len(trajs[0][0]), len(cols)
    d = [lib.DeviceArray.from_host(np.ascontiguousarray(np.concatenate([t[k] for t in trajs])).reshape(-1)) for k in range(3)]
    d_idx = lib.DeviceArray.from_host(np.asarray(cols, dtype=np.int32))
    d_stack = None if R_stack is None else lib.DeviceArray.from_host(np.ascontiguousarray(R_stack).reshape(-1))
    d_R = lib.DeviceArray.from_host(np.full(B * r * r, np.nan))
    assert lib.regressor_tsqr_batch_fused(robot.device_model(), flags, B, n_per, d[0], d[1], d[2], d_idx, r, d_stack, d_R)
    return d_R.to_host().reshape(B, r, r)


def _columnwise(lib, record_property, name, param, B, n_per, stacked, seed, robot=None, cols=None):
    from figaroh_plus_amd.tools.regressor import build_regressor_basic
    robot = robot or _robot(name)
    cols = _base_columns_numpy(robot, param) if cols is None else cols
    r = len(cols)
    trajs = _trajectories(robot, B, n_per, seed)
    R_stack, G0 = None, np.zeros((r, r), dtype=np.longdouble)
    if stacked:
        qs, vs, as_ = _trajectories(robot, 1, 200, seed + 1)[0]
        Ws = build_regressor_basic(robot, qs, vs, as_, dict(param))[:, cols]
        R_stack = np.triu(np.linalg.qr(Ws, mode="r"))
        G0 = _gram_ld(R_stack)
    R = _run_entry(lib, robot, param, trajs, cols, R_stack)
    S = _slices(B, n_per, lib.device_info()["cu_count"])
    for b in sorted({0, B // 2, B - 1}):
        q, v, a = trajs[b]
        W = build_regressor_basic(robot, q, v, a, dict(param))
        assert W.shape == (robot.model.nv * n_per, 14 * robot.model.nv)
        _check_gram(R[b], G0 + _gram_ld(W[:, cols]), record_property,
                    "fusedbatch_%s_r%d_B%d_n%d_S%d_%d_b%d" % (name, r, B, n_per, S, stacked, b))
    return S


@pytest.mark.parametrize("name", ["ur10", "chain5", "chain7"])
@pytest.mark.parametrize("flags", FLAG_SETS, ids=lambda f: "".join(k[4] for k, v in f.items() if v) or "none")
def test_batch_fused_columnwise_flag_sets(lib, name, flags, record_property):
    """Every friction / actuator-inertia / offset flag set (up to four more live columns per link) on the 5-, 6- and 7-joint kernels:
    B = 5 different trajectories of 333 samples (ragged last tile, S > 1), stacked under a previous triangle."""
    S = _columnwise(lib, record_property, name, _param(**flags), 5, 333, True, 11)
    assert S > 1


# (B, n_per, stacked): the floor (one tile, S == 1 however few trajectories); B = 1 cut into many slices, ragged; a batch in
# the hundreds that fills the chip by itself (S == 1, 16 sample tiles per workgroup, ragged); a few long trajectories
# (S > 1, several tiles per slice, three merge levels); 65 samples: a second tile of one live lane
SHAPE_CASES = [(3, N_FLOOR, True), (1, 1000, False), (1, 1000, True), (300, 1001, True), (300, 517, False), (7, 4133, False),
               (2, 65, True), (64, 130, False)]


@pytest.mark.parametrize("B,n_per,stacked", SHAPE_CASES)
def test_batch_fused_columnwise_shapes(lib, B, n_per, stacked, record_property):
    """UR10, the golden's 36 base columns, over the launch shapes: n_per at the floor and not a multiple of 64, S == 1 and
    S > 1, B = 1 and B in the hundreds (first, middle and last trajectory), with and without R_stack."""
    from conftest import Golden
    from figaroh_plus_amd.tools.excitation import base_columns
    g = Golden("cfg2_ur10")
    cols = base_columns(84, g["idx_e"], g["idx_base"])
    assert len(cols) == 36
    S = _columnwise(lib, record_property, "ur10", dict(g.param), B, n_per, stacked, 100 + B, robot=g.robot(), cols=cols)
    record_property("slices", str(S))


def test_shape_cases_reach_every_path():
    """The (B, n_per) choices cover S == 1 by the floor and by B >= CUs, S > 1 with one and with several tiles per slice, and
    one, two and three merge levels (256 CUs, six consumers, 36 columns)."""
    S = {(B, n): _slices(B, n, 256) for B, n, _ in SHAPE_CASES}
    assert S[(3, 64)] == 1 and S[(300, 1001)] == 1 and S[(1, 1000)] == 16 and S[(7, 4133)] == 36 and S[(64, 130)] == 3
    assert _consumers(6, 36) == 6 and _consumers(5, 64) >= 3 and _consumers(7, 63) == 3 and _consumers(7, 64) == 2
    assert _merge_levels(1, 6, 36, True) == 1 and _merge_levels(16, 6, 36, True) == 2 and _merge_levels(36, 6, 36, False) == 3


@pytest.mark.parametrize("name,n_per,B,stacked", [("ur10", 1000, 6, False), ("ur10", 130, 3, True), ("ur10", 64, 7, True),
                                                  ("chain5", 333, 4, True), ("chain7", 517, 3, False)])
def test_objective_cond_batch_fused_matches_numpy_cond(lib, oracle_lib, name, n_per, B, stacked):
    """objective_cond_batch through the fused entry against objective_cond per trajectory (the two-launch path) and against
    np.linalg.cond of the oracle's host W_b (the reference side never touches the HIP kernels), |got - ref| <= 1e-9 ref."""
    from figaroh_plus_amd.tools.excitation import base_regressor_triangle, objective_cond, objective_cond_batch
    robot = _robot(name)
    if name == "ur10":
        from conftest import Golden
        g = Golden("cfg2_ur10")
        param, idx_e, idx_base = dict(g.param), g["idx_e"], g["idx_base"]
    else:
        param = _param(has_friction=True)
        cols = _base_columns_numpy(robot, param)
        ncols = 14 * robot.model.nv
        # (idx_e / idx_base in the reference's two-step numbering: eliminated columns, then positions among the kept)
        qs, vs, as_ = _trajectories(robot, 1, 400, 5)[0]
        from figaroh_plus_amd.tools.regressor import build_regressor_basic
        W = build_regressor_basic(robot, qs, vs, as_, dict(param))
        idx_e = np.flatnonzero(np.sqrt((W * W).sum(axis=0)) <= 1e-6)
        kept = [i for i in range(ncols) if i not in set(idx_e.tolist())]
        idx_base = np.asarray([kept.index(int(c)) for c in cols])
    gone = set(int(i) for i in idx_e)
    om = oracle_lib.OracleModel(robot.model.to_flat())
    mode, fl, ft = oracle_lib.param_flags(param, False)

    def oracle_Wb(q, v, a):
        W = om.build_regressor_basic(q, v, a, mode, fl, ft)
        keep = [i for i in range(W.shape[1]) if i not in gone]
        return W[:, keep][:, idx_base]

    trajs = _trajectories(robot, B, n_per, 7 * n_per + B)
    R_stack, W_stack = None, None
    if stacked:
        qs, vs, as_ = _trajectories(robot, 1, 200, 3)[0]
        W_stack = oracle_Wb(qs, vs, as_)
        R_stack = base_regressor_triangle(robot, qs, vs, as_, param, idx_e, idx_base)
    lib.profile_enable(level=2)
    lib.profile_reset()
    try:
        got = objective_cond_batch(robot, trajs, param, idx_e, idx_base, R_stack=R_stack)
        assert lib.profile_get("fused_chain_tsqr_batch")[0] == 1  # (the fused entry took it, not the fall-back)
    finally:
        lib.profile_enable(False)
    assert len(got) == B
    for b, (q, v, a) in enumerate(trajs):
        Wb = oracle_Wb(q, v, a)
        if stacked:
            Wb = np.vstack((W_stack, Wb))
        ref = np.linalg.cond(Wb)
        one = objective_cond(robot, q, v, a, param, idx_e, idx_base, R_stack=R_stack)
        print("%s b=%d: batch %.12g one %.12g numpy %.12g" % (name, b, got[b], one, ref))
        assert abs(got[b] - ref) <= 1e-9 * ref, (b, got[b], ref)
        assert abs(got[b] - one) <= 1e-9 * ref, (b, got[b], one)


def test_batch_fused_is_one_pass(lib):
    """The point of the entry: for B = 8 and B = 64 trajectories of 1000 UR10 samples there is exactly one level-0 launch, no
    K1 launch, and the same number of merge launches (S = 16 and S = 4: two levels each)."""
    from conftest import Golden
    from figaroh_plus_amd.tools.excitation import base_columns
    g = Golden("cfg2_ur10")
    robot = g.robot()
    cols = base_columns(84, g["idx_e"], g["idx_base"])
    counts = {}
    lib.profile_enable(level=2)
    try:
        for B in (8, 64):
            trajs = _trajectories(robot, B, 1000, B)
            lib.profile_reset()
            _run_entry(lib, robot, dict(g.param), trajs, cols)
            assert lib.profile_get("fused_chain_tsqr_batch")[0] == 1
            assert lib.profile_get("regressor_chain")[0] == 0 and lib.profile_get("fused_chain_tsqr")[0] == 0
            assert lib.profile_get("tsqr")[0] == 0
            counts[B] = lib.profile_get("tsqr_reduce")[0] + lib.profile_get("tsqr_group")[0]
    finally:
        lib.profile_enable(False)
    assert counts[8] == counts[64] and 1 <= counts[8] <= 3, counts


def test_batch_fused_refusals_and_fallback(lib, record_property):
    """Every FIGH_ERR_UNSUPPORTED cause of figh.h one by one through the raw entry: the code, an error text, nothing
    launched; and base_regressor_triangles_batch behind it still returns the right triangles for TX40 and TIAGo."""
    from conftest import Golden
    from figaroh_plus_amd.tools.excitation import base_columns, base_regressor_triangles_batch
    from figaroh_plus_amd.tools.regressor import add_coupling_TX40, build_regressor_basic, regressor_flags
    raw = lib.load().figh_regressor_tsqr_batch_fused
    ur10, tiago = Golden("cfg2_ur10").robot(), Golden("cfg3_tiago").robot()
    chain8, chain7 = _robot("chain8"), _robot("chain7")

    def call(robot, flags, B, n_per, n):
        # (every buffer has the size the shape asks for: a call that were not refused would stay inside them)
        d_q = lib.DeviceArray.from_host(np.zeros(B * n_per * robot.model.nq))
        d_v = lib.DeviceArray.from_host(np.zeros(B * n_per * robot.model.nv))
        d_idx = lib.DeviceArray.from_host(np.arange(n, dtype=np.int32))
        d_R = lib.DeviceArray((B * n * n,), np.float64)
        return raw(robot.device_model().handle, flags, B, n_per, d_q.ptr, d_v.ptr, d_v.ptr, d_idx.ptr, n, None, d_R.ptr)

    causes = [("tree", tiago, 0, 2, 128, 36), ("eight joints", chain8, 0, 2, 128, 36),
              ("tx40 flag", ur10, lib.FLAG_TX40, 2, 128, 36), ("generic flag", ur10, lib.FLAG_GENERIC, 2, 128, 36),
              ("blocked inputs", ur10, lib.FLAG_BLOCKED_INPUTS, 2, 128, 36), ("n = 65", ur10, 0, 2, 128, 65), ("seven joints, n = 64", chain7, 0, 2, 128, 64),
              ("n_per below the floor", ur10, 0, 2, N_FLOOR - 1, 36), ("B above the grid", ur10, 0, 65536, N_FLOOR, 36)]
    lib.profile_enable(level=2)
    try:
        for tag, robot, flags, B, n_per, n in causes:
            lib.profile_reset()
            assert call(robot, flags, B, n_per, n) == lib.ERR_UNSUPPORTED, tag
            assert b"fused batch" in lib.load().figh_last_error(), tag
            for scope in ("fused_chain_tsqr_batch", "tsqr_reduce", "regressor_chain", "tsqr"):
                assert lib.profile_get(scope)[0] == 0, (tag, scope)
        lib.profile_reset()
        assert call(ur10, 0, 2, N_FLOOR, 36) == 0 and lib.profile_get("fused_chain_tsqr_batch")[0] == 1
    finally:
        lib.profile_enable(False)
    # the fall-back: TX40 (coupling columns) and TIAGo (a tree) through excitation.py
    for cfg, B, n_per in (("cfg1_tx40", 2, 517), ("cfg3_tiago", 2, 155)):
        g = Golden(cfg)
        robot = g.robot()
        trajs = _trajectories(robot, B, n_per, 31)
        mode, flags, _ = regressor_flags(g.param, g.coupling)
        rps, ncols = robot.device_model().shape(mode, flags)
        cols = base_columns(ncols, g["idx_e"], g["idx_base"])
        lib.profile_enable(level=2)
        lib.profile_reset()
        try:
            R = base_regressor_triangles_batch(robot, trajs, g.param, g["idx_e"], g["idx_base"], coupling=g.coupling)
            assert lib.profile_get("fused_chain_tsqr_batch")[0] == 0
        finally:
            lib.profile_enable(False)
        for b, (q, v, a) in enumerate(trajs):
            W = build_regressor_basic(robot, q, v, a, dict(g.param))
            if g.coupling:
                m = robot.model
                W = add_coupling_TX40(W, m, robot.data, n_per, m.nq, m.nv, m.njoints, q, v, a)
            _check_gram(R[b], _gram_ld(W[:, cols]), record_property, "fallback_%s_b%d" % (cfg, b))
