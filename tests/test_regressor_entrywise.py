"""GPU suite: the kernels that PRODUCE the regressor W -- the chain kernel (figh_regressor.hip), the tape kernel in all its
layouts (figh_regressor_tree.hip) and the producer half of the fused launch (figh_fused.hip) -- entry by entry against the
long-double reference of tests/regressor_exact.py.

Assertion everywhere: |W - W_ld| <= C_TOL u S for every entry (S: the a-priori error scale of that entry, regressor_exact's
docstring), exact zeros where S == 0, the copied columns (Ia fv fs off, TX40 coupling) equal to their inputs.  C_TOL = 8 x
the largest ratio of the two CPU oracles (regressor_exact.C_ORACLE), not a figure of the kernels.  The inputs cover what the
norm-wise checks of test_gpu_parity.py cannot see: slow and fast trajectories, one moving joint, all four in one wave,
revolute angles up to 2^40 and at multiples of pi / 2, long prismatic strokes and a far-away floating base.  Every case
reports its ratio through record_property.

Measured on an MI355X (C_TOL = 256): chain kernel at most 8.9, tape kernel 10.4 on the shipped models and 16.9 on the random
trees, pipeline layouts 16.8, fused producer 9.7.  Before sincos_angle (figh_spatial.h) reduced angles beyond 2^30 rad itself,
regime bigq gave 8e11 in all three kernel families: the device library's sincos was off by |q| 2^-53 there; now at most 6.2.
"""
import numpy as np
import pytest

import regressor_exact as rx

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 209]
PIPE_REGIMES = ["static", "mixed", "fast"]
FLAG_SETS = [dict(has_friction=bool(f & 1), has_actuator_inertia=bool(f & 2), has_joint_offset=bool(f & 4)) for f in range(8)]
ALL_FLAGS = dict(friction=True, inertia=True, offset=True)


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    return _lib


def _check(W, ref, record_property, what):
    ratio = rx.assert_entrywise(W, ref, rx.C_TOL, what)
    record_property("entry_ratio " + what, round(ratio, 2))
    print("entry_ratio %-60s %.2f" % (what, ratio))
    return ratio


def _chain(name):
    """(robot, key of the flat model for regressor_exact.reference, coupling)."""
    from figaroh_plus_amd.tools.robot import Robot
    if name in ("tx40", "ur10"):
        return Robot.from_flat(name), name, name == "tx40"
    from test_gpu_parity import _synthetic_chain
    robot = _synthetic_chain(int(name[5:]))
    return robot, rx.register(name, robot.model.to_flat()), False


def _tree(shape, freeflyer):
    from test_gpu_parity import _TREES, _synthetic_tree
    parents = _TREES[shape]
    if freeflyer:
        parents = [0] + [p + 1 for p in parents]  # the tree hangs off the free-flyer root
        massless = (6, 9) if shape in ("fork", "caterpillar") else ()
        robot = _synthetic_tree(parents, seed=3 + len(parents), massless=massless, freeflyer=True)
    else:
        robot = _synthetic_tree(parents, seed=len(parents), massless=(4,) if shape == "fork" else ())
    return robot, rx.register(shape + ("-ff" if freeflyer else ""), robot.model.to_flat())


def _drop_in(robot, q, v, a, param, coupling=False, generic=False):
    from figaroh_plus_amd.tools.regressor import add_coupling_TX40, build_regressor_basic
    p = dict(param, force_generic_kernel=True) if generic else dict(param)
    W = build_regressor_basic(robot, q, v, a, p)
    if coupling:
        m = robot.model
        W = add_coupling_TX40(W, m, robot.data, len(q), m.nq, m.nv, m.njoints, q, v, a)
    return W


# ------------------------------------------------------------------------------------------------ chain kernel, drop-in
@pytest.mark.parametrize("regime", rx.REGIMES)
@pytest.mark.parametrize("name", ["tx40", "ur10"] + ["chain%d" % nj for nj in range(1, 9)])
def test_chain_kernel_every_link_count(lib, name, regime, record_property):
    """regressor_chain_kernel for every instantiated link count (1 .. 8; the TX40 with its coupling columns appended), full,
    ragged and single-sample tiles."""
    robot, key, coupling = _chain(name)
    param = rx.base_param(**ALL_FLAGS)
    for N in SIZES:
        (q, v, a), ref = rx.reference(key, regime, N, param, coupling)
        W = _drop_in(robot, q, v, a, param, coupling)
        _check(W, ref, record_property, "chain %s %s N=%d" % (name, regime, N))


@pytest.mark.parametrize("regime", rx.REGIMES)
def test_chain_kernel_tx40_coupling_fused_and_padded_rows(lib, regime, record_property):
    """The TX40 instantiation that writes the coupling columns itself (build_regressor_device(coupling=True), 87 columns), and
    the UR10 rows with a padded leading dimension (the scalar store path): padding untouched."""
    from figaroh_plus_amd.tools.regressor import build_regressor_device, regressor_flags
    from figaroh_plus_amd.tools.robot import Robot
    param = rx.base_param(**ALL_FLAGS)
    N = 209
    robot = Robot.from_flat("tx40")
    (q, v, a), ref = rx.reference("tx40", regime, N, param, True)
    dq, dv, da = (lib.DeviceArray.from_host(np.ascontiguousarray(x).reshape(-1)) for x in (q, v, a))
    W, _ = build_regressor_device(robot, dq, dv, da, N, param, coupling=True, colsq=True)
    Wh = W.numpy()
    assert Wh.shape == (6 * N, 87)
    _check(Wh, ref, record_property, "chain tx40 coupling fused %s" % regime)
    robot = Robot.from_flat("ur10")
    (q, v, a), ref = rx.reference("ur10", regime, N, param)
    dq, dv, da = (lib.DeviceArray.from_host(np.ascontiguousarray(x).reshape(-1)) for x in (q, v, a))
    ldw = 91
    dW = lib.DeviceArray.from_host(np.full(6 * N * ldw, -7.0))
    mode, flags, ft = regressor_flags(param)
    lib.regressor_build(robot.device_model(), mode, flags, ft, N, dq, dv, da, dW, ldw, None)
    Wp = dW.to_host().reshape(6 * N, ldw)
    assert np.all(Wp[:, 84:] == -7.0)
    _check(Wp[:, :84], ref, record_property, "chain ur10 ldw=91 %s" % regime)


@pytest.mark.parametrize("regime", rx.REGIMES)
@pytest.mark.parametrize("flags", FLAG_SETS, ids=lambda f: "".join(k[4] for k, val in f.items() if val) or "none")
def test_chain_kernel_all_flag_sets(lib, flags, regime, record_property):
    from figaroh_plus_amd.tools.robot import Robot
    param = dict(rx.base_param(), **flags)
    robot = Robot.from_flat("ur10")
    (q, v, a), ref = rx.reference("ur10", regime, 65, param)
    _check(_drop_in(robot, q, v, a, param), ref, record_property, "chain ur10 flags %s" % regime)


@pytest.mark.parametrize("regime", rx.REGIMES)
@pytest.mark.parametrize("name", ["tx40", "ur10"])
def test_chain_kernel_main_loop_and_ragged_tail(lib, name, regime, record_property):
    """N = 128 grid + 5 (grid: the workgroup count of launch_chain, CUs x 3 x 2): every workgroup runs the prefetching main
    loop over two full tiles, the first one the ragged last tile as well.  The reference is formed for a subset of samples:
    the first and last tile of the first and last workgroup, the ragged tile, and 1 500 samples at random."""
    from figaroh_plus_amd.tools.regressor import build_regressor_device
    robot, key, coupling = _chain(name)
    param = rx.base_param(**ALL_FLAGS)
    grid = lib.device_info()["cu_count"] * 3 * 2
    N = 128 * grid + 5
    flat = rx.flat_of(key)
    q, v, a = rx.inputs(flat, N, regime, seed=9)
    rng = np.random.default_rng(grid)
    tiles = [0, 1, grid - 1, grid, grid + 1, 2 * grid - 1]
    sel = np.concatenate([64 * t + np.arange(64) for t in tiles] + [np.arange(128 * grid, N), rng.choice(N, 1500, replace=False)])
    sel = np.unique(sel)
    ref = rx.regressor_ld(flat, q[sel], v[sel], a[sel], param, coupling)
    dq, dv, da = (lib.DeviceArray.from_host(np.ascontiguousarray(x).reshape(-1)) for x in (q, v, a))
    W, _ = build_regressor_device(robot, dq, dv, da, N, param, coupling=coupling)
    rows = (np.arange(6)[:, None] * N + sel[None, :]).reshape(-1)
    Wsel = W.numpy()[rows]
    del W
    _check(Wsel, ref, record_property, "chain %s %s N=%d (%d samples)" % (name, regime, N, len(sel)))


# --------------------------------------------------------------------------------------------- tape kernel, drop-in form
@pytest.mark.parametrize("regime", rx.REGIMES)
@pytest.mark.parametrize("name", ["tx40", "ur10"])
def test_tape_kernel_on_chains(lib, name, regime, record_property):
    robot, key, coupling = _chain(name)
    param = rx.base_param(**ALL_FLAGS)
    for N in SIZES:
        (q, v, a), ref = rx.reference(key, regime, N, param, coupling)
        W = _drop_in(robot, q, v, a, param, coupling, generic=True)
        _check(W, ref, record_property, "tape %s %s N=%d" % (name, regime, N))


TAPE_CASES = [("tiago", rx.base_param(**ALL_FLAGS)), ("tiago", rx.base_param()),
              ("talos", rx.base_param(wrench=True)), ("talos", rx.base_param(wrench=True, force_torque=("Fx", "Mz"), **ALL_FLAGS)),
              ("human", rx.base_param(wrench=True)), ("human", rx.base_param(wrench=True, force_torque=("Fx", "Mz"), **ALL_FLAGS))]


@pytest.mark.parametrize("regime", rx.REGIMES)
@pytest.mark.parametrize("name,param", TAPE_CASES, ids=["%s-%d" % (c[0], i) for i, c in enumerate(TAPE_CASES)])
def test_tape_kernel_reference_layout(lib, name, param, regime, record_property):
    """The shipped trees through build_regressor_basic: TIAGo (joint torques), TALOS and the human model (external wrench,
    all six components and Fx + Mz), sample-major inputs."""
    from figaroh_plus_amd.tools.robot import Robot
    robot = Robot.from_flat(name)
    for N in (1, 65, 209):
        (q, v, a), ref = rx.reference(name, regime, N, param)
        _check(_drop_in(robot, q, v, a, param), ref, record_property, "tape %s %s N=%d" % (name, regime, N))


@pytest.mark.parametrize("regime", rx.REGIMES)
@pytest.mark.parametrize("flags", [{}, ALL_FLAGS], ids=["plain", "fv-Ia-off"])
@pytest.mark.parametrize("freeflyer", [False, True], ids=["fixed", "floating"])
@pytest.mark.parametrize("shape", ["binary15", "caterpillar", "chain13", "fork", "star"])
def test_tape_kernel_random_trees(lib, shape, freeflyer, flags, regime, record_property):
    """The trees of test_tree_walks_random_trees_against_oracle / test_freeflyer_walk_state_copy_on_random_trees (every shape
    the windowing of the torque walk distinguishes; nested and sibling branches and massless links under a free-flyer)."""
    robot, key = _tree(shape, freeflyer)
    param = rx.base_param(wrench=freeflyer, **flags)
    N = 64 * 3 + 17
    (q, v, a), ref = rx.reference(key, regime, N, param)
    _check(_drop_in(robot, q, v, a, param), ref, record_property, "tape tree %s %s" % (key, regime))


# ------------------------------------------------------------------------------------------- tape kernel, pipeline layouts
def _pipeline_W(lib, robot, param, qva, layout, row_blocks=None, seed=0):
    """The reference-layout W of the second pass of an IdentificationPipeline in layout ``layout`` (tile-blocked inputs),
    read back through the column maps of qr_graded_common; rows of inactive row blocks are returned as NaN."""
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from qr_graded_common import read_wrench_layout
    q, v, a = qva
    N, m = len(q), robot.model
    nl = m.njoints - 1
    rps = m.nv if param["is_joint_torques"] else 6
    nb = rps if row_blocks is None else len(row_blocks)
    tau = np.random.default_rng(seed).standard_normal(nb * N)
    pipe = IdentificationPipeline(robot, param, row_blocks=row_blocks, w_layout=layout)
    pipe.set_samples(q, v, a, tau)
    assert pipe._in_flags == lib.FLAG_BLOCKED_INPUTS
    pipe.run()
    pipe.run()
    buf = pipe.W.buf.to_host()
    if getattr(pipe, "_compact", None) is not None:
        off, ld = pipe._compact
        W = np.zeros((rps * N, 14 * nl))
        for row in range(rps):
            if row_blocks is not None and row not in row_blocks:
                assert ld[row] == 0
                W[row * N:(row + 1) * N] = np.nan
                continue
            j = int(np.flatnonzero(np.array([jm.idx_v for jm in m.joints[1:]]) == row)[0])  # first link of the window
            blk = buf[off[row]:off[row] + N * ld[row]].reshape(N, ld[row])
            nlk = ld[row] // 16
            assert not blk.reshape(N, nlk, 16)[:, :, 14:].any()
            W[row * N:(row + 1) * N, 14 * j:14 * (j + nlk)] = blk.reshape(N, nlk, 16)[:, :, :14].reshape(N, 14 * nlk)
        return W, "block-compact"
    link_pos = getattr(pipe, "_link_pos", None)
    ldf = getattr(pipe, "_force_ld", 0)
    W = read_wrench_layout(buf, rps * N, 14 * nl, pipe.W.ld, 16, link_pos, ldf)
    kind = ("force-compact" if ldf else "one-matrix") + (" link-compact" if link_pos is not None else " link-padded")
    return W, kind


@pytest.mark.parametrize("regime", PIPE_REGIMES)
@pytest.mark.parametrize("layout,blocks", [("link-padded", None), ("block-compact", None), ("block-compact", "even")])
def test_tape_kernel_pipeline_layouts_tiago(lib, layout, blocks, regime, record_property):
    from figaroh_plus_amd.tools.robot import Robot
    robot = Robot.from_flat("tiago")
    param = rx.base_param(**ALL_FLAGS)
    N = 209
    row_blocks = None if blocks is None else list(range(0, robot.model.nv, 2))
    (q, v, a), ref = rx.reference("tiago", regime, N, param, seed=1)
    W, kind = _pipeline_W(lib, robot, param, (q, v, a), layout, row_blocks)
    assert kind == ("block-compact" if layout == "block-compact" else "one-matrix link-padded")
    if row_blocks is not None:  # the blocks that are not stored are not compared
        live = np.repeat(np.isin(np.arange(robot.model.nv), row_blocks), N)
        assert np.all(np.isnan(W[~live])) and not np.isnan(W[live]).any()
        W, ref = W[live], rx.Ref(ref.W[live], ref.S[live], ref.copied)
    _check(W, ref, record_property, "pipeline tiago %s %s %s" % (layout, blocks, regime))


@pytest.mark.parametrize("regime", PIPE_REGIMES)
@pytest.mark.parametrize("layout", ["link-padded", "link-compact", "dense"])
@pytest.mark.parametrize("name", ["talos", "human"])
def test_tape_kernel_pipeline_layouts_wrench(lib, name, layout, regime, record_property):
    """External-wrench regressor in the pipeline's layouts: link-padded, link-compact (one matrix; the human model has
    massless links, TALOS none: the layout must then not engage) and the default, force-compact (the free-flyer walk with
    the state copy at branch joints)."""
    from figaroh_plus_amd.tools.robot import Robot
    robot = Robot.from_flat(name)
    param = rx.base_param(wrench=True)
    N = 64 * 50 + 23  # (the force-compact layout wants 16 (ncols + 1) / 3 samples)
    (q, v, a), ref = rx.reference(name, regime, N, param, seed=1)
    W, kind = _pipeline_W(lib, robot, param, (q, v, a), layout)
    want = {"link-padded": "one-matrix link-padded", "link-compact": "one-matrix link-compact", "dense": "force-compact link-compact"}[layout]
    if name == "talos":
        want = want.replace("link-compact", "link-padded")
    if layout == "dense" and regime == "static":
        # (slow samples: the columns the pass keeps do not allow the force / torque split, and the pipeline keeps this
        # regressor as one matrix -- its documented fallback; the other two regimes run the force-compact walk)
        assert kind in (want, want.replace("force-compact", "one-matrix")), kind
    else:
        assert kind == want, kind
    _check(W, ref, record_property, "pipeline %s %s %s" % (name, kind, regime))


@pytest.mark.parametrize("regime", PIPE_REGIMES)
@pytest.mark.parametrize("shape", ["binary15", "fork"])
def test_tape_kernel_pipeline_layouts_random_trees(lib, shape, regime, record_property):
    """Block-compact row blocks of a fixed-base tree and the force-compact walk (state copy at nested and sibling branch
    joints) of the same tree under a free-flyer."""
    robot, key = _tree(shape, False)
    param = rx.base_param(**ALL_FLAGS)
    (q, v, a), ref = rx.reference(key, regime, 209, param, seed=2)
    W, kind = _pipeline_W(lib, robot, param, (q, v, a), "block-compact")
    assert kind == "block-compact"
    _check(W, ref, record_property, "pipeline tree %s block-compact %s" % (key, regime))
    robot, key = _tree(shape, True)
    param = rx.base_param(wrench=True)
    del W, ref
    (q, v, a), ref = rx.reference(key, regime, 64 * 40 + 23, param, seed=2)
    W, kind = _pipeline_W(lib, robot, param, (q, v, a), "dense")
    assert kind.startswith("force-compact") or regime == "static", kind  # (static: one matrix, as above)
    _check(W, ref, record_property, "pipeline tree %s %s %s" % (key, kind, regime))


# ------------------------------------------------------------------------------------------------------- fused launch
@pytest.mark.parametrize("regime", ["static", "mixed", "bigq"])
@pytest.mark.parametrize("N", [4096, 20037])
@pytest.mark.parametrize("name", ["ur10", "chain5", "chain7"])
def test_fused_launch_producer(lib, name, N, regime, record_property):
    """The producer half of figh_regressor_tsqr_fused (it re-forms the link rotations per row: code of its own): W of the
    second, fused pass, written again after the buffer was poisoned."""
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    robot, key, _ = _chain(name)
    param = rx.base_param()
    (q, v, a), ref = rx.reference(key, regime, N, param, seed=3)
    tau = np.random.default_rng(N).standard_normal(robot.model.nv * N)
    pipe = IdentificationPipeline(robot, param, fuse=True)
    pipe.set_samples(q, v, a, tau)
    pipe.run()
    lib.check(lib.load().figh_memset(pipe.W.buf.ptr, 0xff, pipe.W.rows * pipe.W.ld * 8))
    pipe.run()
    assert pipe.fused_passes == 2, "the second pass did not take the fused launch"
    W = np.empty((pipe.W.rows, pipe.W.ld))
    lib.check(lib.load().figh_memcpy_d2h(W.ctypes.data, pipe.W.buf.ptr, W.nbytes))
    _check(W[:, :ref.W.shape[1]], ref, record_property, "fused %s %s N=%d" % (name, regime, N))
