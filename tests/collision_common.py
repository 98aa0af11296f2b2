"""Shared by test_collision_host.py (CPU) and test_collision_distances.py (GPU): the case tables of the self-collision
distances and a CERTIFICATE of a returned distance that owes nothing to GJK.

For a query with returned d, witness points pA, pB (world frame, on the cores) and status OK:
  1. membership: pA lies in core A and pB in core B -- each point is mapped to the shape's local frame through a forward
     kinematics the test owns (``placed`` below: calibration_tools._world_placements, composed here; test_collision_host
     ties it to the mpmath restatement of kinematics_common) and the shape's inequalities are tested with allowance delta;
  2. d + r_A + r_B = |pA - pB| to 4 units in the last place of the largest number involved (the coordinates, r_A + r_B and
     |d| -- the subtraction of the radii rounds at that magnitude, not at |pA - pB|'s);
  3. with n = (pB - pA) / |pB - pA|:  lb = min_{y in B} n.y - max_{x in A} n.x from the closed-form support VALUES below
     (any unit n gives a lower bound), hence lb <= dist(core_A, core_B) <= |pA - pB|;
  4. |pA - pB| - lb <= tol + delta.
From 3 and 4 a device and a mirror that both pass agree to |d_dev - d_mir| <= tol + 2 delta: derived, not measured.

delta is the rounding of the check itself, with S the largest coordinate in play (world translations plus shape extents, at
least 1): the float64 forward kinematics composes at most 2 * 8 placements (TIAGo's deepest geometry chain is six joints, the
free-flyer tree's four) at 3 products and 2 sums per entry, the geometry placement and the map to the local frame are three
more such products, the support values and the norm a dozen operations: below 128 roundings of numbers of size S on the test's
side, and as many on the side under test for its own kinematics and witness sums.  delta = 256 u S; ``delta_for`` asserts
delta < tol / 100.
"""
import json
import os
import types

import numpy as np

import kinematics_common as kc
from figaroh_plus_amd.calibration.calibration_tools import _mul, _se3_tuple, _world_placements
from figaroh_plus_amd.model import SE3
from figaroh_plus_amd.tools import robotcollisions as rc

U = 2.0 ** -53
SENTINEL = -3.25e55
TOL = rc.DEFAULT_TOL
KINDS = (rc.KIND_BOX, rc.KIND_CYLINDER, rc.KIND_SPHERE, rc.KIND_CAPSULE)
KIND_PAIRS = [(a, b) for a in KINDS for b in KINDS if a <= b]  # the ten unordered pairs
GAPS = (1e-1, 1e-3, 1e-6)
GPU_N = (1, 63, 64, 65, 130)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiago_simplified_collision.json")


def delta_for(S, tol=TOL):
    delta = 256.0 * U * max(1.0, float(S))
    assert delta < tol / 100.0, (delta, tol)
    return delta


# ------------------------------------------------------------------------------------------------------- shapes and poses
def make_shape(kind, dims):
    if kind == rc.KIND_BOX:
        return rc.Box(*dims[:3])
    if kind == rc.KIND_SPHERE:
        return rc.Sphere(dims[0])
    return (rc.Cylinder if kind == rc.KIND_CYLINDER else rc.Capsule)(*dims[:2])


def random_shape(rng, kind):
    """Sizes of 5 to 30 cm."""
    return make_shape(kind, rng.uniform(0.05, 0.3, size=3))


def random_rotations(rng, M):
    q = rng.normal(size=(M, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    x, y, z, w = q.T
    R = np.empty((M, 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)
    return R


def random_poses(rng, M):
    """Rotations uniform, positions within +-0.6 m."""
    return random_rotations(rng, M), rng.uniform(-0.6, 0.6, size=(M, 3))


def half_of(shape):
    return rc.core_half_extents(shape.kind, shape.dimensions)


def gjk(shape_a, Ra, pa, shape_b, Rb, pb, tol=TOL, max_iter=rc.DEFAULT_MAX_ITER):
    """The mirror's GJK on placed shapes: (d, pA, pB, status, iterations)."""
    core, pA, pB, st, it = rc.gjk_core_distance(shape_a.kind, half_of(shape_a), Ra, pa, shape_b.kind, half_of(shape_b), Rb, pb,
                                                tol, max_iter)
    return core - (shape_a.core_radius + shape_b.core_radius), pA, pB, st, it


# --------------------------------------------------------------------------------- the test's own closed forms of a core
def support_value(shape, R, p, n):
    """max over the core of n.x, for unit vectors n (M, 3): n.p + the core's extent along R^T n."""
    nl = np.einsum("mrc,mr->mc", R, n)
    k = shape.kind
    if k == rc.KIND_BOX:
        ext = np.abs(nl) @ shape.halfSide
    elif k == rc.KIND_CYLINDER:
        ext = shape.radius * np.hypot(nl[:, 0], nl[:, 1]) + shape.halfLength * np.abs(nl[:, 2])
    elif k == rc.KIND_SPHERE:
        ext = np.zeros(len(nl))
    else:
        ext = shape.halfLength * np.abs(nl[:, 2])
    return np.einsum("mr,mr->m", n, p) + ext


def outside_by(shape, R, p, x):
    """How far (metres, >= 0) the world points x (M, 3) violate the inequalities of the placed core."""
    xl = np.einsum("mrc,mr->mc", R, x - p)
    k = shape.kind
    if k == rc.KIND_BOX:
        return np.max(np.abs(xl) - shape.halfSide, axis=1).clip(min=0.0)
    if k == rc.KIND_CYLINDER:
        return np.maximum(np.hypot(xl[:, 0], xl[:, 1]) - shape.radius, np.abs(xl[:, 2]) - shape.halfLength).clip(min=0.0)
    if k == rc.KIND_SPHERE:
        return np.linalg.norm(xl, axis=1)
    return np.maximum(np.hypot(xl[:, 0], xl[:, 1]), np.abs(xl[:, 2]) - shape.halfLength).clip(min=0.0)


def surface_samples(shape, n=60):
    """Dense samples of the local surface of a core, for the check of ``support_value``."""
    k = shape.kind
    t = np.linspace(-1.0, 1.0, n)
    if k == rc.KIND_BOX:
        g = np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1).reshape(-1, 3)
        return g[np.max(np.abs(g), axis=1) == 1.0] * shape.halfSide
    if k == rc.KIND_SPHERE:
        return np.zeros((1, 3))
    z = t * shape.halfLength
    if k == rc.KIND_CAPSULE:
        return np.stack((0 * z, 0 * z, z), axis=-1)
    ang = np.linspace(0.0, 2 * np.pi, 40 * n, endpoint=False)
    side = np.stack(np.broadcast_arrays(shape.radius * np.cos(ang)[:, None], shape.radius * np.sin(ang)[:, None], z[None, :]),
                    axis=-1).reshape(-1, 3)
    rad = np.linspace(0.0, shape.radius, n)
    caps = [np.stack(np.broadcast_arrays(rad[None, :] * np.cos(ang)[:, None], rad[None, :] * np.sin(ang)[:, None], s),
                     axis=-1).reshape(-1, 3) for s in (-shape.halfLength, shape.halfLength)]
    return np.concatenate([side] + caps)


# -------------------------------------------------------------------------------------------------------- the certificate
def certify(shape_a, Ra, pa, shape_b, Rb, pb, d, pA, pB, status, tol=TOL, tag=""):
    """Asserts 1 - 4 of the module docstring on the queries whose status is OK; returns (upper, lower bound) of the core
    distance of every query (lb <= dist <= ub whatever the status, when the witnesses lie in the cores)."""
    S = max(np.abs(pa).max(), np.abs(pb).max()) + np.abs(half_of(shape_a)).sum() + np.abs(half_of(shape_b)).sum()
    delta = delta_for(S, tol)
    rr = shape_a.core_radius + shape_b.core_radius
    ok = status == rc.STATUS_OK
    ub = np.linalg.norm(pA - pB, axis=1)
    out_a, out_b = outside_by(shape_a, Ra, pa, pA), outside_by(shape_b, Rb, pb, pB)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = (pB - pA) / ub[:, None]
    n = np.where(ub[:, None] > 0.0, n, np.array([1.0, 0.0, 0.0]))
    lb = -support_value(shape_b, Rb, pb, -n) - support_value(shape_a, Ra, pa, n)
    lb = np.where(ub > 0.0, lb, -np.inf)
    print("%s: %d queries, %d OK; worst membership %.3g / %.3g, worst |pA - pB| - lb %.3g (tol %.3g + delta %.3g)"
          % (tag, len(d), ok.sum(), out_a.max(), out_b.max(), (ub - lb)[ok].max() if ok.any() else 0.0, tol, delta))
    assert np.all(out_a[ok] <= delta) and np.all(out_b[ok] <= delta), (tag, "membership", out_a[ok].max(), out_b[ok].max())
    big = np.maximum(np.maximum(np.abs(pA).max(axis=1), np.abs(pB).max(axis=1)), np.maximum(rr, np.abs(d)))
    assert np.all(np.abs((d + rr) - ub)[ok] <= 4 * np.spacing(big)[ok]), (tag, "d + r_A + r_B != |pA - pB|")
    assert np.all((ub - lb)[ok] <= tol + delta), (tag, "duality gap", (ub - lb)[ok].max())
    return ub, lb


# ----------------------------------------------------------------------------------------------- robots with geometries
def placed(model, geom_model, q):
    """The test's own forward kinematics: [(R (N, 3, 3), p (N, 3))] = oM_parent . placement of every geometry object."""
    q = np.atleast_2d(np.asarray(q, dtype=np.float64))
    objs = geom_model.geometryObjects
    oM = _world_placements(model, q, [o.parentJoint for o in objs])
    out = []
    for o in objs:
        R, p = _mul(oM[o.parentJoint][1], _se3_tuple(o.placement))
        out.append((np.broadcast_to(R, (len(q), 3, 3)).copy(), np.broadcast_to(p, (len(q), 3)).copy()))
    return out


def placed_exact(model, geom_model, q_row):
    """The same placements of ONE configuration from the mpmath restatement of kinematics_common, as float64."""
    objs = geom_model.geometryObjects
    oM = kc.world(model, q_row, [o.parentJoint for o in objs])
    out = []
    for o in objs:
        M = kc.mat_mul(oM[o.parentJoint][1], kc.hom_of_se3(o.placement))
        out.append((np.array([[float(M[r][c].v) for c in range(3)] for r in range(3)]),
                    np.array([float(M[r][3].v) for r in range(3)])))
    return out


def certify_model(model, geom_model, q, d, pA, pB, status, tol=TOL, tag=""):
    """``certify`` pair by pair for distances (N, n_pairs) of a robot's geometry model; returns (ub, lb) (N, n_pairs)."""
    P = placed(model, geom_model, q)
    ub, lb = np.zeros(d.shape), np.zeros(d.shape)
    for k, pair in enumerate(geom_model.collisionPairs):
        oa, ob = geom_model.geometryObjects[pair.first], geom_model.geometryObjects[pair.second]
        ub[:, k], lb[:, k] = certify(oa.geometry, *P[pair.first], ob.geometry, *P[pair.second], d[:, k], pA[:, k], pB[:, k],
                                     status[:, k], tol, "%s %s-%s" % (tag, oa.name, ob.name))
    return ub, lb


def delta_model(model, geom_model, q, tol=TOL):
    P = placed(model, geom_model, q)
    S = max(np.abs(p).max() for _, p in P) + max(np.abs(half_of(o.geometry)).sum() for o in geom_model.geometryObjects)
    return delta_for(S, tol)


def configurations(model, n, seed):
    return kc.Case.configurations(types.SimpleNamespace(model=model), n, seed)


def _offset(seed):
    rng = np.random.default_rng(seed)
    from figaroh_plus_amd.model import rpy_to_matrix
    return SE3(rpy_to_matrix(*rng.uniform(-1.0, 1.0, 3)), rng.uniform(-0.1, 0.1, 3))


def tiago_case():
    """TIAGo with the committed fixture: objects on the universe, the torso, the arm and the head; four pairs."""
    from figaroh_plus_amd.tools.robot import Robot
    robot = Robot.from_flat("tiago")
    with open(GOLDEN) as f:
        robot.geom_model = rc.GeometryModel.from_dict(json.load(f), robot.model)
    return robot


def ur10_case(n_pairs=4):
    """UR10 (a chain): box, cylinder, sphere, capsule on four links and the base; pairs of unlike kinds."""
    from figaroh_plus_amd.tools.robot import Robot
    robot = Robot.from_flat("ur10")
    m, gm = robot.model, rc.GeometryModel()
    gm.addGeometryObject(rc.GeometryObject("base_box", 0, rc.Box(0.3, 0.3, 0.1), SE3(None, [0.0, 0.0, -0.06])))
    gm.addGeometryObject(rc.GeometryObject("upper_cyl", m.getJointId("shoulder_lift_joint"), rc.Cylinder(0.06, 0.5), _offset(1)))
    gm.addGeometryObject(rc.GeometryObject("elbow_sphere", m.getJointId("elbow_joint"), rc.Sphere(0.08), _offset(2)))
    gm.addGeometryObject(rc.GeometryObject("wrist_cap", m.getJointId("wrist_2_joint"), rc.Capsule(0.05, 0.2), _offset(3)))
    gm.addGeometryObject(rc.GeometryObject("tool_box", m.getJointId("wrist_3_joint"), rc.Box(0.1, 0.08, 0.15), _offset(4)))
    for a, b in (("base_box", "wrist_cap"), ("upper_cyl", "tool_box"), ("base_box", "elbow_sphere"), ("upper_cyl", "wrist_cap"),
                 )[:n_pairs]:
        gm.addCollisionPair(rc.CollisionPair(gm.getGeometryId(a), gm.getGeometryId(b)))
    robot.geom_model = gm
    return robot


def tree_case():
    """The free-flyer tree of the kinematics tests (revolute root, continuous, free-flyer, prismatic, a revolute side branch;
    placements that are not the identity), one object on the root joint; the like-kind pairs the robots above leave out."""
    from figaroh_plus_amd.tools.robot import Robot
    m = kc._tree()
    robot = Robot(None, _model=m)
    gm = rc.GeometryModel()
    gm.addGeometryObject(rc.GeometryObject("root_cyl", m.getJointId("r1"), rc.Cylinder(0.2, 0.3), _offset(11)))
    gm.addGeometryObject(rc.GeometryObject("fly_sphere", m.getJointId("ff3"), rc.Sphere(0.1), _offset(12)))
    gm.addGeometryObject(rc.GeometryObject("fly_cap", m.getJointId("ff3"), rc.Capsule(0.05, 0.3), _offset(13)))
    gm.addGeometryObject(rc.GeometryObject("slide_box", m.getJointId("p4"), rc.Box(0.2, 0.1, 0.3), _offset(14)))
    gm.addGeometryObject(rc.GeometryObject("side_sphere", m.getJointId("r5"), rc.Sphere(0.12), _offset(15)))
    gm.addGeometryObject(rc.GeometryObject("side_cap", m.getJointId("r5"), rc.Capsule(0.04, 0.25), _offset(16)))
    gm.addGeometryObject(rc.GeometryObject("world_box", 0, rc.Box(0.3, 0.3, 0.3), SE3(None, [0.5, 0.0, 0.0])))
    for a, b in (("fly_sphere", "side_sphere"), ("fly_cap", "side_cap"), ("slide_box", "world_box"), ("root_cyl", "fly_sphere"),
                 ("root_cyl", "slide_box"), ("fly_sphere", "side_cap"), ("world_box", "fly_sphere"), ("world_box", "fly_cap")):
        gm.addCollisionPair(rc.CollisionPair(gm.getGeometryId(a), gm.getGeometryId(b)))
    robot.geom_model = gm
    return robot


def kind_pairs_of(*robots):
    out = set()
    for r in robots:
        for p in r.geom_model.collisionPairs:
            ka, kb = (r.geom_model.geometryObjects[i].geometry.kind for i in (p.first, p.second))
            out.add((min(ka, kb), max(ka, kb)))
    return out
