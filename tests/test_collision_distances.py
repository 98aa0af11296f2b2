"""GPU suite: figh_collision_distances (csrc/figh_collision.hip) and the Python layer on top of it.  The device's distances
pass the certificate of tests/collision_common.py (independent of GJK) and agree with the NumPy mirror to the bound that
follows from it, |d_dev - d_mir| <= tol + 2 delta; every output is the tail of a wider, sentinel-filled row buffer whose head
and padding are asserted untouched; end to end, evaluate_waypoints_batch(..., collision=cw) appends the distances to rows
whose first part is bit-equal to the call without them and moves no sample array across the bus."""
import functools

import numpy as np
import pytest

import collision_common as cc
import trajectory_common as tc
from figaroh_plus_amd.tools import robotcollisions as rc

pytestmark = pytest.mark.gpu
HEAD, PAD = 3, 2


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    return _lib


def _run(lib, robot, q, B, n_per, idx=None, tol=cc.TOL, max_iter=rc.DEFAULT_MAX_ITER, witness=True, status=True, gm=None):
    """The raw entry on sentinel-filled buffers: the distances land HEAD doubles into rows of HEAD + n + PAD doubles, one
    spare row behind; returns (d (B, n_eval, n_pairs), pA, pB, status, iterations), the optional ones None when not asked."""
    gm = robot.geom_model if gm is None else gm
    m = robot.model
    P = len(gm.collisionPairs)
    n_eval = n_per if idx is None else len(idx)
    n, ldq = n_eval * P, m.nq + 2
    ld = HEAD + n + PAD
    qp = np.full((B * n_per, ldq), cc.SENTINEL)
    qp[:, :m.nq] = q
    d_q = lib.DeviceArray.from_host(qp.reshape(-1))
    d_out = lib.DeviceArray.from_host(np.full((B + 1) * ld, cc.SENTINEL))
    d_w = lib.DeviceArray.from_host(np.full(6 * B * n + 6, cc.SENTINEL)) if witness else None
    d_s = lib.DeviceArray.from_host(np.full(B * n + 1, -77, dtype=np.int32)) if status else None
    rc.collision_distances_device(robot, gm, d_q.ptr, ldq, B, n_per, idx, d_out.ptr + 8 * HEAD, ld, tol, max_iter,
                                  d_w.ptr if witness else None, d_s.ptr if status else None)
    full = d_out.to_host().reshape(B + 1, ld)
    assert np.all(full[:B, :HEAD] == cc.SENTINEL) and np.all(full[:B, HEAD + n:] == cc.SENTINEL) and np.all(full[B] == cc.SENTINEL)
    assert not np.any(full[:B, HEAD:HEAD + n] == cc.SENTINEL)
    d = full[:B, HEAD:HEAD + n].reshape(B, n_eval, P)
    pA = pB = st = it = None
    if witness:
        w = d_w.to_host()
        assert np.all(w[6 * B * n:] == cc.SENTINEL)
        w = w[:6 * B * n].reshape(B, n_eval, P, 6)
        pA, pB = w[..., :3], w[..., 3:]
    if status:
        s = d_s.to_host()
        assert s[B * n] == -77
        s = s[:B * n].reshape(B, n_eval, P)
        st, it = s & 0xFFFF, s >> 16
    return d, pA, pB, st, it


CASES = {"ur10_one_pair": lambda: cc.ur10_case(1), "ur10": cc.ur10_case, "tiago": cc.tiago_case, "tree": cc.tree_case}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(robot, q, mirror results) for max(GPU_N) configurations, computed once; smaller N take the first rows."""
    robot = CASES[name]()
    q = cc.configurations(robot.model, max(cc.GPU_N), 17)
    return robot, q, rc.collision_distances_mirror(robot.model, robot.geom_model, q)


def _compare(robot, q, got, ref, tag, tol=cc.TOL):
    d, pA, pB, st, it = got
    d_m, _, _, st_m, it_m = ref
    delta = cc.delta_model(robot.model, robot.geom_model, q, tol)
    ub, lb = cc.certify_model(robot.model, robot.geom_model, q, d, pA, pB, st, tol, tag)
    print("%s: worst |d_dev - d_mir| %.3g (bound %.3g); iterations device max %d mean %.2f, mirror max %d; statuses %s"
          % (tag, np.abs(d - d_m).max(), tol + 2 * delta, it.max(), it.mean(), it_m.max(), np.bincount(st.ravel(), minlength=3)))
    assert np.all(np.abs(d - d_m) <= tol + 2 * delta), (tag, np.abs(d - d_m).max())
    assert np.all((st == st_m) | (ub <= tol)), tag
    assert not np.any(st == rc.STATUS_ITERATION_CAP), tag
    cut = st == rc.STATUS_CORES_INTERSECT
    rr = np.array([robot.geom_model.geometryObjects[p.first].geometry.core_radius
                   + robot.geom_model.geometryObjects[p.second].geometry.core_radius for p in robot.geom_model.collisionPairs])
    assert np.array_equal(d[cut], np.broadcast_to(-rr, d.shape)[cut]), tag


def test_cases_cover_every_kind_pair():
    assert cc.kind_pairs_of(*(CASES[n]() for n in CASES)) == set(cc.KIND_PAIRS)
    assert sorted({len(CASES[n]().geom_model.collisionPairs) for n in CASES}) == [1, 4, 8]


@pytest.mark.parametrize("N", cc.GPU_N)
@pytest.mark.parametrize("name", list(CASES))
def test_device_certified_and_within_the_mirror_bound(lib, name, N):
    robot, q, ref = _reference(name)
    got = _run(lib, robot, q[:N], 1, N)
    _compare(robot, q[:N], tuple(x[0] for x in got), tuple(x[:N] for x in ref), "%s N=%d" % (name, N))


@pytest.mark.parametrize("B", [1, 3])
def test_sample_subsets_and_every_sample(lib, B):
    robot, q, ref = _reference("tiago")
    n_per = 7
    rows = q[:B * n_per]
    every = _run(lib, robot, rows, B, n_per)
    flat = tuple(x.reshape((B * n_per,) + x.shape[2:]) for x in every)
    _compare(robot, rows, flat, tuple(x[:B * n_per] for x in ref), "tiago B=%d every sample" % B)
    idx = [2, 6]  # a strict subset with the last sample
    sub = _run(lib, robot, rows, B, n_per, idx=idx)
    for got, want in zip(sub, every):
        assert got.shape[1] == 2 and np.array_equal(got, want[:, idx])
    one = _run(lib, robot, rows, B, n_per, idx=[6, 0, 6])  # (any order, repeats allowed)
    assert np.array_equal(one[0], every[0][:, [6, 0, 6]])


def test_optional_outputs_and_identical_bits(lib):
    robot, q, _ = _reference("tree")
    full = _run(lib, robot, q[:65], 1, 65)
    again = _run(lib, robot, q[:65], 1, 65)
    assert all(np.array_equal(a, b) for a, b in zip(full, again))
    no_w = _run(lib, robot, q[:65], 1, 65, witness=False)
    no_s = _run(lib, robot, q[:65], 1, 65, status=False)
    neither = _run(lib, robot, q[:65], 1, 65, witness=False, status=False)
    assert no_w[1] is None and no_s[3] is None
    assert np.array_equal(no_w[0], full[0]) and np.array_equal(no_w[3], full[3]) and np.array_equal(no_w[4], full[4])
    assert np.array_equal(no_s[0], full[0]) and np.array_equal(no_s[1], full[1]) and np.array_equal(no_s[2], full[2])
    assert np.array_equal(neither[0], full[0])


def test_iteration_cap_is_reported_and_still_an_upper_bound(lib):
    """max_iter = 2: the bounded loop ends, the call returns normally, the statuses say ITERATION_CAP and the values are upper
    bounds (lb <= d_core, witnesses in the cores)."""
    robot, q, ref = _reference("tiago")
    d, pA, pB, st, it = (x[0] for x in _run(lib, robot, q[:65], 1, 65, max_iter=2))
    assert np.all(it <= 2) and np.all(it >= 1)
    cap = st == rc.STATUS_ITERATION_CAP
    assert cap.sum() > cap.size // 2 and not np.any(st == rc.STATUS_OK)  # (box / cylinder pairs need more than two steps)
    ub, lb = cc.certify_model(robot.model, robot.geom_model, q[:65], d, pA, pB, st, tag="max_iter 2")
    delta = cc.delta_model(robot.model, robot.geom_model, q[:65])
    assert np.all(lb[cap] <= ub[cap]) and np.all(ub[cap] >= ref[0][:65][cap] - cc.TOL - delta)
    big = np.maximum(np.abs(pA).max(axis=2), np.abs(pB).max(axis=2))  # (the fixture's shapes are their own cores: d = |pA - pB|,
    assert np.all(np.abs(d - ub)[cap] <= 4 * np.spacing(big)[cap])    # to the rounding of item 2 of the certificate)
    P = cc.placed(robot.model, robot.geom_model, q[:65])
    for k, pair in enumerate(robot.geom_model.collisionPairs):
        oa, ob = (robot.geom_model.geometryObjects[i] for i in (pair.first, pair.second))
        assert np.all(cc.outside_by(oa.geometry, *P[pair.first], pA[:, k]) <= delta)
        assert np.all(cc.outside_by(ob.geometry, *P[pair.second], pB[:, k]) <= delta)


def test_refusals_launch_nothing(lib):
    robot, q, _ = _reference("tiago")
    m, gm = robot.model, robot.geom_model
    kind, parent, placement, dims, pairs, _ = rc.geometry_table(gm)
    n_per, P = 5, len(pairs)
    d_q = lib.DeviceArray.from_host(q[:2 * n_per].reshape(-1))
    d_out = lib.DeviceArray.from_host(np.full(2 * n_per * P, cc.SENTINEL))
    d_w = lib.DeviceArray.from_host(np.full(6 * 2 * n_per * P, cc.SENTINEL))
    d_s = lib.DeviceArray.from_host(np.full(2 * n_per * P, -77, dtype=np.int32))

    def call(idx=None, kind=kind, parent=parent, placement=placement, dims=dims, pairs=pairs, tol=1e-9, max_iter=128,
             ld_b=n_per * P, ldq=m.nq, B=2):
        lib.collision_distances(robot.device_model(), B, n_per, idx, d_q.ptr, ldq, kind, parent, placement, dims, pairs, tol,
                                max_iter, d_out.ptr, ld_b, d_w.ptr, d_s.ptr)

    many_g = rc.MAX_GEOMETRIES + 1
    cases = [("too many pairs", dict(pairs=np.tile(pairs, (17, 1))[:rc.MAX_PAIRS + 1])),
             ("no pair", dict(pairs=np.zeros((0, 2), dtype=np.int32))),
             ("too many objects", dict(kind=np.zeros(many_g, dtype=np.int32), parent=np.zeros(many_g, dtype=np.int32),
                                       placement=np.tile(placement[0], (many_g, 1)), dims=np.ones((many_g, 3)))),
             ("max_iter 0", dict(max_iter=0)), ("max_iter 1025", dict(max_iter=1025)), ("tol 0", dict(tol=0.0)),
             ("tol negative", dict(tol=-1e-9)), ("tol nan", dict(tol=float("nan"))),
             ("pair off the table", dict(pairs=np.array([[0, 3], [1, 5]]))), ("pair negative", dict(pairs=np.array([[-1, 3]]))),
             ("pair with itself", dict(pairs=np.array([[3, 3]]))), ("index n_per", dict(idx=[0, n_per])),
             ("index negative", dict(idx=[-1])), ("unknown kind", dict(kind=np.array([0, 0, 1, 4, 1]))),
             ("parent off the model", dict(parent=np.array([13, 13, 0, m.njoints, 24]))),
             ("row stride", dict(ld_b=n_per * P - 1)), ("ldq", dict(ldq=m.nq - 1)), ("B 0", dict(B=0))]
    lib.profile_enable(level=2)
    try:
        lib.profile_reset()
        for tag, kw in cases:
            with pytest.raises(lib.FighError) as e:
                call(**kw)
            assert e.value.code == lib.ERR_INVALID, tag
        assert lib.profile_get("collision_distances")[0] == 0
        assert np.all(d_out.to_host() == cc.SENTINEL) and np.all(d_w.to_host() == cc.SENTINEL) and np.all(d_s.to_host() == -77)
        call()
        assert lib.profile_get("collision_distances")[0] == 1 and not np.any(d_out.to_host() == cc.SENTINEL)
    finally:
        lib.profile_enable(False)


def test_wrapper_routes_agree_with_the_entry(lib):
    from figaroh_plus_amd.device import GpuMatrix
    robot, q, ref = _reference("ur10")
    raw = _run(lib, robot, q[:64], 1, 64)
    cw = rc.CollisionWrapper(robot)
    hit = cw.computeCollisions(GpuMatrix.from_host(q[:64]))
    assert np.array_equal(cw.getDistances(), raw[0][0]) and np.array_equal(cw.getStatus(), raw[3][0])
    assert np.array_equal(hit, np.any(raw[0][0] <= 0.0, axis=1))
    assert np.array_equal(cw.computeCollisions(q[:64]), hit) and np.array_equal(cw.getDistances(), raw[0][0])
    assert cw.computeCollisions(q[5]) == bool(hit[5]) and np.array_equal(cw.getDistances(), raw[0][0][5])


def test_evaluate_waypoints_batch_with_collision_rows(lib, monkeypatch):
    """TIAGo, the eight script joints, B = 4, 5 waypoints, 61 samples: the first part of every row is bit-equal to the call
    without ``collision``, the tail is within the mirror bound, n_con grows by (n_wps - 1) n_pairs, and no array of B n_per
    entries per active joint or more crosses the bus except the (B, n_con) result and the B r x r triangles."""
    from conftest import Golden
    from figaroh_plus_amd.device import GpuMatrix
    from figaroh_plus_amd.tools import excitation as ex
    from test_trajectory_exact import _indices_from_spline
    g = Golden("cfg3_tiago")
    robot = cc.tiago_case()
    robot.q0 = tc.model_case("tiago_arm")[2]
    cs = ex.CubicSpline(robot, 5, tc.MODEL_CASES["tiago_arm"][1])
    param = dict(g.param)
    idx_e, idx_base = _indices_from_spline(robot, lambda n: ex.CubicSpline(robot, n, tc.MODEL_CASES["tiago_arm"][1]), param)
    tps, B, n_per = [0.0, 0.15, 0.3, 0.45, 0.6], 4, 61
    rng = np.random.default_rng(23)
    n_act, n_wps = cs.dim_q
    wp_init = rng.uniform(-0.3, 0.3, size=n_act)
    lo, up = np.maximum(cs.lower_q, -1.5), np.minimum(cs.upper_q, 1.5)
    X = rng.uniform(np.tile(lo, n_wps - 1), np.tile(up, n_wps - 1), size=(B, (n_wps - 1) * n_act))
    vel, acc = 0.3 * rng.normal(size=(n_act, n_wps)), rng.normal(size=(n_act, n_wps))
    cw = rc.CollisionWrapper(robot)
    conds0, cons0 = ex.evaluate_waypoints_batch(robot, cs, 100, tps, X, vel, acc, wp_init, param, idx_e, idx_base)
    up_sizes, down_sizes = [], []
    from_host, to_host = lib.DeviceArray.from_host.__func__, lib.DeviceArray.to_host

    def rec_up(cls, arr, dtype=None):
        up_sizes.append(int(np.asarray(arr).size))
        return from_host(cls, arr, dtype)

    def rec_down(self, out=None):
        down_sizes.append(self.size)
        return to_host(self, out)

    def no_matrix_download(self):
        raise AssertionError("GpuMatrix.numpy() inside the resident route")

    monkeypatch.setattr(lib.DeviceArray, "from_host", classmethod(rec_up))
    monkeypatch.setattr(lib.DeviceArray, "to_host", rec_down)
    monkeypatch.setattr(GpuMatrix, "numpy", no_matrix_download)
    conds, cons = ex.evaluate_waypoints_batch(robot, cs, 100, tps, X, vel, acc, wp_init, param, idx_e, idx_base, collision=cw)
    monkeypatch.undo()
    idx = ex.waypoint_sample_indices(ex.spline_times(100, tps)[3], tps)
    P = len(robot.geom_model.collisionPairs)
    n_con = cons0.shape[1]
    assert len(idx) == n_wps - 1 and n_con == len(idx) * n_act + 2 * n_per * n_act
    assert cons.shape == (B, n_con + (n_wps - 1) * P)
    assert np.array_equal(cons[:, :n_con], cons0) and conds == conds0
    r = len(idx_base)
    # the instrument of test_evaluate_waypoints_batch_moves_no_sample_array; at this small shape (B n_per = 244) the model's
    # 336 standard parameters are longer than one column of samples, so a sample array is counted from its true smallest
    # size, B n_per entries for each of the n_act active joints (q, v, a and tau are all wider)
    sample_array = B * n_per * n_act
    assert up_sizes and max(up_sizes) < sample_array, up_sizes
    assert sorted(x for x in down_sizes if x >= sample_array) == sorted([B * cons.shape[1], B * r * r]), down_sizes
    wps = ex.waypoints_from_search_variables(X, wp_init, n_wps, n_act)
    cl, cu = ex.constraint_bounds(cs, n_wps, n_per, n_pairs=P)
    assert len(cl) == len(cu) == cons.shape[1]
    for b in range(B):
        _, p, _, _ = cs.get_full_config(100, np.array(tps).reshape(-1, 1), wps[b], vel, acc)
        want = rc.collision_distances_mirror(robot.model, robot.geom_model, p[idx])[0]
        delta = cc.delta_model(robot.model, robot.geom_model, p[idx])
        tail = cons[b, n_con:].reshape(n_wps - 1, P)
        print("trajectory %d: worst |tail - mirror| %.3g" % (b, np.abs(tail - want).max()))
        assert np.all(np.abs(tail - want) <= cc.TOL + 2 * delta)
    batch = ex.spline_batch(cs, 100, tps, wps, vel, acc)
    alone = ex.collision_distances_batch(robot, batch, idx)
    assert np.array_equal(alone, cons[:, n_con:])
    assert ex.collision_distances_batch(robot, batch, None).shape == (B, n_per * P)
