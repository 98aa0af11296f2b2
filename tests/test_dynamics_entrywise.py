"""GPU suite: figh_regressor_apply -- tau = W(q, v, a) . phi without W (csrc/figh_dynamics.hip) -- row by row against the
long-double W . phi of tests/dynamics_exact.py.

Assertion everywhere: |tau - tau_ld| <= C_TAU u T for every row (T: the a-priori error scale of the row, dynamics_exact's
docstring) and exact zeros where T == 0.  C_TAU = 8 x the largest ratio of the float64 NumPy restatement of the algorithm
(dynamics_exact.C_TAU_ORACLE), not a figure of the kernels.  Every case reports its ratio through record_property.  One
long-double reference per (model, regime, flags) at 209 samples; the smaller sizes are its leading samples.

Measured on an MI355X (C_TAU = 128; 360 cases in 15 s): chain kernel at most 5.8 (UR10, mixed), tree kernel 6.3 on the shipped
models (TIAGo, static) and 7.2 on the random trees (caterpillar, static), the tree kernel on the chains 5.8, persistent grid
2.0 (UR10) and 3.6 (TIAGo) at N = 131 153, the mirrors against the fallback path 3.5 (get_torque_rand) and 1.0 (calc_torque).
"""
import numpy as np
import pytest

import dynamics_exact as dx
import regressor_exact as rx

pytestmark = pytest.mark.gpu

N_REF = 209
CHAIN_SIZES = [1, 63, 64, 65, 209]
TREE_SIZES = [1, 64, 65, 209]
ALL_FLAGS = dict(friction=True, inertia=True, offset=True)
FLAG_SETS = [dict(has_friction=bool(f & 1), has_actuator_inertia=bool(f & 2), has_joint_offset=bool(f & 4)) for f in range(8)]


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    return _lib


def _report(record_property, what, ratio):
    record_property("tau_ratio " + what, round(ratio, 2))
    print("tau_ratio %-64s %.2f" % (what, ratio))


def _check(tau, tau_ld, T, record_property, what):
    ratio = dx.assert_tau(tau, tau_ld, T, dx.C_TAU, what)
    _report(record_property, what, ratio)
    return ratio


def _leading(x, rows, n):
    """The rows of the first n of N_REF samples of a stacked (rows N_REF) vector."""
    return x.reshape(rows, N_REF)[:, :n].reshape(-1)


def _chain(name):
    from test_regressor_entrywise import _chain as chain
    return chain(name)


def _tree(shape, freeflyer):
    from test_regressor_entrywise import _tree as tree
    return tree(shape, freeflyer)


def _apply(robot, q, v, a, param, phi, coupling=False, **kw):
    from figaroh_plus_amd.tools.regressor import regressor_times_parameters
    return regressor_times_parameters(robot, q, v, a, param, phi, coupling=coupling, **kw)


def _sweep(robot, key, regime, param, phi, coupling, sizes, record_property, what):
    """One reference at N_REF samples; the device at every size in ``sizes`` on its leading samples."""
    (q, v, a), ref = rx.reference(key, regime, N_REF, param, coupling)
    tau_ld, T = dx.tau_from_ref(ref, phi)
    rows = len(T) // N_REF
    for n in sizes:
        tau = _apply(robot, q[:n], v[:n], a[:n], param, phi, coupling)
        assert tau.shape == (rows * n,) and tau.dtype == np.float64
        _check(tau, _leading(tau_ld, rows, n), _leading(T, rows, n), record_property, "%s %s N=%d" % (what, regime, n))


# ------------------------------------------------------------------------------------------------------------- chains
@pytest.mark.parametrize("regime", rx.REGIMES)
@pytest.mark.parametrize("name", ["tx40", "ur10"] + ["chain%d" % nj for nj in range(1, 9)])
def test_chain_kernel_every_link_count(lib, name, regime, record_property):
    """inverse_dynamics_chain_kernel for every instantiated link count (the TX40 with its coupling columns): full, ragged and
    single-sample tiles, all flags, the model's own phi."""
    robot, key, coupling = _chain(name)
    nl = robot.model.njoints - 1
    param = dx.drive_param(rx.base_param(**ALL_FLAGS), nl)
    phi = dx.phi_of(rx.flat_of(key), param, coupling)
    _sweep(robot, key, regime, param, phi, coupling, CHAIN_SIZES, record_property, "chain " + name)


@pytest.mark.parametrize("regime", rx.REGIMES)
@pytest.mark.parametrize("flags", FLAG_SETS, ids=lambda f: "".join(k[4] for k, val in f.items() if val) or "none")
def test_chain_kernel_all_flag_sets(lib, flags, regime, record_property):
    """All eight flag sets at N = 65.  The entries of phi that belong to a flag that is off are NaN on the device: they must not
    be read."""
    from figaroh_plus_amd.tools.robot import Robot
    robot = Robot.from_flat("ur10")
    flat = rx.flat_of("ur10")
    on = dict(has_friction=True, has_actuator_inertia=True, has_joint_offset=True)
    full = dx.phi_of(flat, dx.drive_param(dict(rx.base_param(), **on), 6))
    param = dict(rx.base_param(), **flags)
    slot = np.arange(84) % 14
    unused = ((slot == 10) & (not flags["has_actuator_inertia"])) | (((slot == 11) | (slot == 12)) & (not flags["has_friction"])) \
        | ((slot == 13) & (not flags["has_joint_offset"]))
    (q, v, a), ref = rx.reference("ur10", regime, 65, param)
    tau_ld, T = dx.tau_from_ref(ref, np.where(unused, 0.0, full))
    tau = _apply(robot, q, v, a, param, np.where(unused, np.nan, full))
    _check(tau, tau_ld, T, record_property, "chain ur10 flags %s" % regime)


# -------------------------------------------------------------------------------------------------------------- trees
TREE_CASES = [("tiago", rx.base_param(**ALL_FLAGS)), ("tiago", rx.base_param()),
              ("talos", rx.base_param(wrench=True)), ("talos", rx.base_param(wrench=True, **ALL_FLAGS)),
              ("talos", rx.base_param(wrench=True, force_torque=("Fz", "Mx"))),
              ("talos", rx.base_param(wrench=True, force_torque=("Fz", "Mx"), **ALL_FLAGS)),
              ("human", rx.base_param(wrench=True)), ("human", rx.base_param(wrench=True, **ALL_FLAGS)),
              ("human", rx.base_param(wrench=True, force_torque=("Fz", "Mx"))),
              ("human", rx.base_param(wrench=True, force_torque=("Fz", "Mx"), **ALL_FLAGS))]


@pytest.mark.parametrize("regime", rx.REGIMES)
@pytest.mark.parametrize("name,param", TREE_CASES, ids=["%s-%d" % (c[0], i) for i, c in enumerate(TREE_CASES)])
def test_tree_kernel_shipped_models(lib, name, param, regime, record_property):
    """inverse_dynamics_tree_kernel on TIAGo (joint torques), TALOS and the human model (external wrench, all six components
    and Fz + Mx), with and without the friction / inertia / offset columns."""
    from figaroh_plus_amd.tools.robot import Robot
    robot = Robot.from_flat(name)
    nl = robot.model.njoints - 1
    pp = dx.drive_param(param, nl)
    phi = dx.phi_of(rx.flat_of(name), pp)
    _sweep(robot, name, regime, pp, phi, False, TREE_SIZES, record_property, "tree " + name)


@pytest.mark.parametrize("regime", rx.REGIMES)
@pytest.mark.parametrize("flags", [{}, ALL_FLAGS], ids=["plain", "fv-Ia-off"])
@pytest.mark.parametrize("freeflyer", [False, True], ids=["fixed", "floating"])
@pytest.mark.parametrize("shape", ["binary15", "caterpillar", "chain13", "fork", "star"])
def test_tree_kernel_random_trees(lib, shape, freeflyer, flags, regime, record_property):
    """Every tree shape of test_gpu_parity._TREES, joint torques on a fixed base and the wrench under a free-flyer (nested and
    sibling branches, several roots, massless links); the massless links keep their entries in phi -- joint-torque mode counts
    them, the external-wrench mode must skip them."""
    robot, key = _tree(shape, freeflyer)
    nl = robot.model.njoints - 1
    param = dx.drive_param(rx.base_param(wrench=freeflyer, **flags), nl)
    phi = dx.phi_of(rx.flat_of(key), param, rng=np.random.default_rng(nl))
    massless = np.flatnonzero(np.asarray(rx.flat_of(key)["mass"])[1:] == 0.0)
    for k in massless:  # (the model's own entries are zero there: give them values that would show)
        phi[14 * k:14 * k + 10] = np.random.default_rng(k).uniform(0.5, 2.0, 10)
    _sweep(robot, key, regime, param, phi, False, TREE_SIZES, record_property, "tree " + key)


@pytest.mark.parametrize("regime", rx.REGIMES)
@pytest.mark.parametrize("name", ["tx40", "ur10"])
def test_tree_kernel_on_chains(lib, name, regime, record_property):
    """The tree kernel on the serial chains (FIGH_FLAG_GENERIC), the TX40 with its coupling columns."""
    robot, key, coupling = _chain(name)
    param = dx.drive_param(dict(rx.base_param(**ALL_FLAGS), force_generic_kernel=True), 6)
    phi = dx.phi_of(rx.flat_of(key), param, coupling)
    _sweep(robot, key, regime, param, phi, coupling, [65, 209], record_property, "tree-kernel " + name)


# ---------------------------------------------------------------------------------------------------- persistent grid
@pytest.mark.parametrize("name", ["ur10", "tiago"])
def test_persistent_grid_with_ragged_remainder(lib, name, record_property):
    """N = 64 (waves + 1) + 17 with ``waves`` from the launch rule (_lib.regressor_apply_waves): every wave runs at least one
    tile, the first two a second one, the second of them the ragged last tile -- the per-wave workspace of the tree kernel is
    used again.  The reference is formed for the first and last tiles of the first and last wave, the wrap-around tiles and
    500 samples at random."""
    from figaroh_plus_amd.tools.robot import Robot
    robot = Robot.from_flat(name)
    flat = rx.flat_of(name)
    nl = robot.model.njoints - 1
    waves = lib.regressor_apply_waves(1 << 40)
    assert waves == lib.APPLY_WAVES_PER_CU * lib.device_info()["cu_count"]
    N = 64 * (waves + 1) + 17
    assert lib.regressor_apply_waves(N) == waves and (N + 63) // 64 == waves + 2
    param = dx.drive_param(rx.base_param(**ALL_FLAGS), nl)
    phi = dx.phi_of(flat, param)
    q, v, a = rx.inputs(flat, N, "unit", seed=9)
    rng = np.random.default_rng(waves)
    sel = np.unique(np.concatenate([64 * t + np.arange(64) for t in (0, 1, waves - 1, waves)]
                                   + [np.arange(64 * (waves + 1), N), rng.choice(N, 500, replace=False)]))
    tau_ld, T = dx.tau_from_ref(rx.regressor_ld(flat, q[sel], v[sel], a[sel], param), phi)
    tau = _apply(robot, q, v, a, param, phi)
    assert tau.shape == (nl * N,)
    _check(tau.reshape(nl, N)[:, sel].reshape(-1), tau_ld, T, record_property, "persistent %s N=%d (%d samples)" % (name, N, len(sel)))


# -------------------------------------------------------------------------------------------------- parameter vectors
@pytest.mark.parametrize("name,coupling", [("tx40", True), ("tiago", False), ("talos", False)])
def test_parameter_vectors(lib, name, coupling, record_property):
    """A random signed phi; the ``cols`` form (phi over a subset of the columns) against the full form; a phi that is zero
    except for one link's block: only the rows of that link's ancestors (joint torques) are non-zero."""
    from figaroh_plus_amd.tools.robot import Robot
    robot = Robot.from_flat(name)
    flat = rx.flat_of(name)
    nl = robot.model.njoints - 1
    wrench = name == "talos"
    param = dx.drive_param(rx.base_param(wrench=wrench, **ALL_FLAGS), nl)
    N = 65
    (q, v, a), ref = rx.reference(name, "unit", N, param, coupling)
    phi = dx.phi_of(flat, param, coupling, np.random.default_rng(5))
    tau_ld, T = dx.tau_from_ref(ref, phi)
    _check(_apply(robot, q, v, a, param, phi, coupling), tau_ld, T, record_property, "signed phi " + name)
    cols = np.sort(np.random.default_rng(6).choice(len(phi), len(phi) // 3, replace=False))
    sub = np.zeros(len(phi))
    sub[cols] = phi[cols]
    tau_cols = _apply(robot, q, v, a, param, phi[cols], coupling, cols=cols)
    assert np.array_equal(tau_cols, _apply(robot, q, v, a, param, sub, coupling))
    _check(tau_cols, *dx.tau_from_ref(ref, sub), record_property, "cols form " + name)
    depth = [0] * (nl + 1)
    for j in range(1, nl + 1):
        depth[j] = depth[int(flat["parents"][j])] + 1
    k = int(np.argmax(depth)) - 1
    one = np.zeros(len(phi))
    one[14 * k:14 * k + 10] = phi[14 * k:14 * k + 10]
    tau_one = _apply(robot, q, v, a, param, one, coupling)
    t_ld, t_T = dx.tau_from_ref(ref, one)
    _check(tau_one, t_ld, t_T, record_property, "one link " + name)
    if not wrench:
        anc, j = set(), k + 1
        while j > 0:
            anc.add(j - 1)
            j = int(flat["parents"][j])
        live = set(np.flatnonzero((tau_one.reshape(-1, N) != 0).any(axis=1)))
        assert live == anc and 1 < len(anc), (live, anc)


# ------------------------------------------------------------------------------------ output buffer, determinism, refusals
def _device_inputs(lib, q, v, a):
    return tuple(lib.DeviceArray.from_host(np.ascontiguousarray(x).reshape(-1)) for x in (q, v, a))


@pytest.mark.parametrize("name", ["ur10", "tiago", "talos"])
def test_output_buffer_and_determinism(lib, name):
    """A sentinel behind the last entry stays untouched; two calls give the same bits."""
    from figaroh_plus_amd.tools.regressor import regressor_flags
    from figaroh_plus_amd.tools.robot import Robot
    robot = Robot.from_flat(name)
    nl = robot.model.njoints - 1
    param = dx.drive_param(rx.base_param(wrench=name == "talos", **ALL_FLAGS), nl)
    mode, flags, ft = regressor_flags(param)
    rows, ncols = robot.device_model().shape(mode, flags)
    N = 209
    q, v, a = rx.inputs(rx.flat_of(name), N, "mixed", seed=2)
    dq, dv, da = _device_inputs(lib, q, v, a)
    d_phi = lib.DeviceArray.from_host(dx.phi_of(rx.flat_of(name), param))
    outs = []
    for _ in range(2):
        d_tau = lib.DeviceArray.from_host(np.full(rows * N + 64, -7.25))
        assert lib.regressor_apply(robot.device_model(), mode, flags, ft, N, dq, dv, da, d_phi, d_tau)
        out = d_tau.to_host()
        assert np.all(out[rows * N:] == -7.25) and not np.any(out[:rows * N] == -7.25)
        outs.append(out)
    assert outs[0].tobytes() == outs[1].tobytes()


def _explicit_fallback(lib, robot, dq, dv, da, N, param, phi, extra_flags=0):
    """build_regressor_device + figh_matvec: the parent's only route to W . phi."""
    from figaroh_plus_amd.tools.regressor import build_regressor_device
    W, _ = build_regressor_device(robot, dq, dv, da, N, param, extra_flags=extra_flags)
    d_phi = lib.DeviceArray.from_host(np.ascontiguousarray(phi))
    d_y = lib.DeviceArray((W.rows,), np.float64)
    lib.matvec(W.buf, W.rows, W.ld, None, W.cols, d_phi, d_y)
    return d_y.to_host()


def _launches(lib):
    return lib.profile_get("inverse_dynamics")[0]


def test_refusals_launch_nothing_and_fall_back(lib, oracle_lib, record_property):
    """External wrench on a fixed base and tile-blocked inputs: FIGH_ERR_UNSUPPORTED, no launch, the output untouched -- and
    the Python surface still returns W . phi, through build + figh_matvec."""
    from figaroh_plus_amd.tools.regressor import regressor_flags, regressor_times_parameters, regressor_times_parameters_device
    from figaroh_plus_amd.tools.robot import Robot
    lib.profile_enable(True, 2)
    try:
        lib.profile_reset()
        N = 130
        # (i) external wrench, first joint not a free-flyer
        robot = Robot.from_flat("ur10")
        flat = rx.flat_of("ur10")
        param = rx.base_param(wrench=True)
        mode, flags, ft = regressor_flags(param)
        q, v, a = rx.inputs(flat, N, "unit", seed=4)
        dq, dv, da = _device_inputs(lib, q, v, a)
        phi = dx.phi_of(flat, param)
        d_phi = lib.DeviceArray.from_host(phi)
        d_tau = lib.DeviceArray.from_host(np.full(6 * N, -7.25))
        assert lib.regressor_apply(robot.device_model(), mode, flags, ft, N, dq, dv, da, d_phi, d_tau) is False
        assert b"free-flyer" in lib.load().figh_last_error()
        assert np.all(d_tau.to_host() == -7.25) and _launches(lib) == 0
        tau = regressor_times_parameters(robot, q, v, a, param, phi)
        assert _launches(lib) == 0
        assert np.array_equal(tau, _explicit_fallback(lib, robot, dq, dv, da, N, param, phi))
        om = oracle_lib.OracleModel(flat)
        W_ref = om.build_regressor_basic(q, v, a, *oracle_lib.param_flags(param, False))
        assert np.abs(tau - W_ref @ phi).max() <= 1e-12 * np.abs(W_ref @ phi).max()
        # (ii) tile-blocked inputs
        robot = Robot.from_flat("tiago")
        flat = rx.flat_of("tiago")
        nl = robot.model.njoints - 1
        param = dx.drive_param(rx.base_param(**ALL_FLAGS), nl)
        mode, flags, ft = regressor_flags(param)
        (q, v, a), ref = rx.reference("tiago", "unit", N_REF, param)
        dq, dv, da = _device_inputs(lib, q, v, a)
        bq, bv, ba = (lib.repack_samples(d, N_REF, w) for d, w in ((dq, robot.model.nq), (dv, robot.model.nv), (da, robot.model.nv)))
        phi = dx.phi_of(flat, param)
        d_phi = lib.DeviceArray.from_host(phi)
        d_tau = lib.DeviceArray.from_host(np.full(nl * N_REF, -7.25))
        assert lib.regressor_apply(robot.device_model(), mode, flags | lib.FLAG_BLOCKED_INPUTS, ft, N_REF, bq, bv, ba, d_phi,
                                   d_tau) is False
        assert b"tile-blocked" in lib.load().figh_last_error()
        assert np.all(d_tau.to_host() == -7.25) and _launches(lib) == 0
        tau = regressor_times_parameters_device(robot, bq, bv, ba, N_REF, param, phi, extra_flags=lib.FLAG_BLOCKED_INPUTS).to_host()
        assert _launches(lib) == 0
        assert np.array_equal(tau, _explicit_fallback(lib, robot, bq, bv, ba, N_REF, param, phi, lib.FLAG_BLOCKED_INPUTS))
        tau_ld, T = dx.tau_from_ref(ref, phi)
        # (the fallback sums 336 products of entries that are each within C_TOL u S)
        _report(record_property, "fallback tiago blocked inputs", dx.assert_tau(tau, tau_ld, T, rx.C_TOL + 336, "fallback"))
        # ... and the served shape does launch
        assert lib.regressor_apply(robot.device_model(), mode, flags, ft, N_REF, dq, dv, da, d_phi, d_tau) is True
        assert _launches(lib) == 1
    finally:
        lib.profile_enable(False)


# ------------------------------------------------------------------------------------------------- fallback agreement
def test_mirrors_agree_with_the_fallback_path(lib, record_property):
    """get_torque_rand (all flag blocks and the coupled-wrist statements), calc_torque and calc_torque_batch (B = 3, n_per =
    70) against build + figh_matvec on the same samples: |difference| <= C_TAU u T."""
    from figaroh_plus_amd.tools.excitation import calc_torque, calc_torque_batch
    from figaroh_plus_amd.tools.randomdata import get_torque_rand
    from figaroh_plus_amd.tools.robot import Robot
    robot = Robot.from_flat("tx40")
    flat = rx.flat_of("tx40")
    nv = 6
    B, n_per = 3, 70
    N = B * n_per
    param = dx.drive_param(dict(rx.base_param(**ALL_FLAGS), has_coupled_wrist=True), nv)
    (q, v, a), ref = rx.reference("tx40", "unit", N, rx.base_param(**ALL_FLAGS))
    dq, dv, da = _device_inputs(lib, q, v, a)

    def agree(tau, fb, T, what):
        assert tau.shape == fb.shape == T.shape
        r = float((np.abs(tau - fb) / (rx.U * T)).max())
        _report(record_property, what, r)
        assert r <= dx.C_TAU, (what, r)

    phi = dx.phi_of(flat, param)
    _, T = dx.tau_from_ref(ref, phi)
    fb = _explicit_fallback(lib, robot, dq, dv, da, N, rx.base_param(**ALL_FLAGS), phi)
    s = np.sign(v[:, 4] + v[:, 5])
    fb[4 * N:5 * N] += param["Iam6"] * v[:, 5] + param["fvm6"] * v[:, 5] + param["fsm6"] * s
    fb[5 * N:6 * N] += param["Iam6"] * v[:, 4] + param["fvm6"] * v[:, 4] + param["fsm6"] * s
    agree(get_torque_rand(N, robot, q, v, a, param), fb, T, "get_torque_rand tx40")
    rigid = rx.base_param()
    phi0 = dx.phi_of(flat, rigid)
    _, T0 = dx.tau_from_ref(rx.reference("tx40", "unit", N, rigid)[1], phi0)
    fb0 = _explicit_fallback(lib, robot, dq, dv, da, N, rigid, phi0)
    agree(calc_torque(N, robot, q, v, a, param), fb0, T0, "calc_torque tx40")
    trajs = [(q[b * n_per:(b + 1) * n_per], v[b * n_per:(b + 1) * n_per], a[b * n_per:(b + 1) * n_per]) for b in range(B)]
    out = calc_torque_batch(robot, trajs, param)
    assert out.shape == (B, nv * n_per)
    for b in range(B):
        pick = (np.arange(nv)[:, None] * N + b * n_per + np.arange(n_per)[None, :]).reshape(-1)
        agree(out[b], fb0[pick], T0[pick], "calc_torque_batch tx40 b=%d" % b)
        assert np.array_equal(out[b], calc_torque(n_per, robot, *trajs[b], param))
